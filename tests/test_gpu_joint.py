"""Joint posterior of the batched ranking (abc_rank_targets_joint_dev, abc_particle_ranking_pls_targets_joint, abc_weighted_joint*):
the device against the NumPy long-double reference of the header's definition (tests/_joint_ref.py) evaluated on the device's own
rows, adjusted values, weights, bandwidths and grids.  Every case checks the means, covariances and correlations within their
bounds, grid and bw bit-equal to the marginal densities' at the same arguments, every pair density within the accuracy contract and
the joint mode as the first largest cell of the device's own density.  Then the behaviour of pair lists, bad parameters and given
bandwidths, bit-for-bit invariance, and the argument errors.

The shapes sit at the edges of k_jt_pair's tiling (joint.hip): 4 entries per MFMA step, JT_TILE = 1024 entries per LDS tile, blocks
of 16 x 16 inside a wave's 64 x 64, one wave up to G = 64 and four above; 16 parameters per covariance tile."""
import ctypes as C

import numpy as np
import pytest

import _density_ref as D
import _joint_ref as J

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LD = np.longdouble
WORST = {"rel": 0.0}                       # largest |f_dev - f_ref| / f_ref seen where f_ref >= 1e-280 max f_ref
NAMES = ("mean", "cov", "corr", "dens", "grid", "bw", "mode", "mode_dens")


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


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def _host(r):
    return {k: (_np(v) if v is not None else None) for k, v in r.items()}


def _joint(F, T, K, exclude=None, **kw):
    import torch
    from abcsmc_amd import device
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    r = device.rank_targets_joint(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"], exclude=ex, **kw)
    torch.cuda.synchronize()
    return _host(r)


def _marginal(F, T, K, exclude=None, **kw):
    """grid and bw of the marginal densities at the same arguments"""
    import torch
    from abcsmc_amd import device
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    r = device.rank_targets_density(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"], exclude=ex, dens=False,
                                    mode=False, **kw)
    torch.cuda.synchronize()
    return _host(r)


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def _check_target(v, w, out, G, bw=None):
    """one target: v (K, P), w (K,) or None, out: the device's arrays of this target"""
    v = np.asarray(v, dtype=np.float64)
    K, P = v.shape
    bad = J.bad_parameters(v)
    ref = J.moments(v, w)
    mean, cov, corr = out["mean"], out["cov"], out["corr"]
    assert np.array_equal(np.isnan(mean), bad)
    ok = ~bad
    # a fixed-order sum of K terms
    assert np.all(np.abs(mean[ok].astype(LD) - ref["mean"][ok]) <= K * 2.0 ** -52 * np.abs(v[:, ok]).max(axis=0)), "mean"
    ok2 = ok[:, None] & ok[None, :]
    assert np.array_equal(np.isnan(cov), ~ok2), "cov NaN pattern"
    var = np.diag(ref["cov"])
    scale = np.sqrt(np.outer(var, var))
    assert np.all(np.abs(cov.astype(LD) - ref["cov"])[ok2] <= (LD(1e-9) * scale)[ok2]), "cov"
    assert np.array_equal(cov, cov.T, equal_nan=True) and np.array_equal(corr, corr.T, equal_nan=True), "symmetry"
    defined = ok2 & (np.outer(var, var) > 0)
    assert np.array_equal(np.isnan(corr), ~defined), "corr NaN pattern"
    assert np.all(np.abs(corr.astype(LD) - ref["corr"])[defined] <= 1e-9), "corr"
    assert np.all(np.diag(corr)[np.diag(defined)] == 1.0) and np.all(np.abs(corr[defined]) <= 1.0)
    h, lo_x, step = out["bw"], out["grid"][:, 0], out["grid"][:, 1]
    assert np.array_equal(np.isnan(h), bad) and np.array_equal(np.isnan(lo_x), bad) and np.array_equal(np.isnan(step), bad)
    if bw is not None:
        assert np.array_equal(h[ok], np.broadcast_to(bw, (P,))[ok])
    x = {j: D.grid_points(lo_x[j], step[j], G) for j in range(P) if ok[j]}
    for p, (i, j) in enumerate(out["pairs"]):
        dens, mode, md = out["dens"][p], out["mode"][p], out["mode_dens"][p]
        if bad[i] or bad[j]:
            assert np.isnan(dens).all() and np.isnan(mode).all() and np.isnan(md), (i, j)
            continue
        f_ref = J.pair_density_at(v[:, i], v[:, j], w, x[i], x[j], h[i], h[j])
        err = np.abs(dens.astype(LD) - f_ref)
        big = f_ref >= 1e-280 * f_ref.max()
        WORST["rel"] = max(WORST["rel"], float((err[big] / f_ref[big]).max()))
        assert np.all(err <= J.density_bound(f_ref)), ((i, j), float((err[big] / f_ref[big]).max()))
        g = int(np.argmax(dens))                               # the first on ties, in flat order
        assert mode[0] == x[i][g // G] and mode[1] == x[j][g % G] and md == dens.reshape(-1)[g], ((i, j), mode, md)


def _check_all(vals, wts, out, G, bw=None):
    """vals (B, K, P), wts (B, K) or None, out: the device's arrays with the targets leading"""
    for b in range(vals.shape[0]):
        one = {k: out[k][b] for k in NAMES}
        one["pairs"] = out["pairs"]
        _check_target(vals[b], None if wts is None else wts[b], one, G, bw=None if bw is None else np.asarray(bw)[b])


@pytest.mark.parametrize("N,M,P,K,B,G,excl,pairs", [
    (300, 5, 1, 1, 3, 2, False, None),                          # one parameter: no pairs, the moments alone
    (400, 5, 2, 2, 1, 15, True, None),
    (400, 6, 3, 3, 3, 16, False, None),
    (500, 6, 5, 5, 1, 256, True, [(0, 1), (4, 2)]),             # sixteen blocks of 64 x 64, four work-group chunks
    (600, 6, 3, 63, 20, 17, False, None),                       # one row and one column past a 16 x 16 block
    (500, 6, 3, 5, 2, 129, False, [(0, 2)]),                    # nine blocks in three chunks: the last has one live wave
    (900, 6, 17, 257, 1, 17, True, None),                       # two covariance tiles, 136 pairs
    (3000, 8, 5, 1000, 3, 64, False, [(0, 1), (3, 2)]),         # a full 64 x 64 block
    (3000, 8, 3, 1025, 1, 65, True, [(2, 0)]),                  # one entry past the LDS tile; four blocks, three of them edges
    (3000, 6, 2, 1000, 20, 15, False, None),
])
def test_rejection(ctx, N, M, P, K, B, G, excl, pairs):
    import torch
    from abcsmc_amd import device
    X, Y = _wl(M, P, N, N + K)
    F = _fit(ctx, X, Y, min(M, P))
    rows = np.arange(B) * 3 % N
    ex = rows if excl else None
    r = _joint(F, X[rows], K, exclude=ex, G=G, pairs=pairs, dist=True)
    Td = torch.empty((M, B), dtype=torch.float64, device=DEV)          # (unit stride also with one target)
    Td.copy_(torch.tensor(X[rows]).T)
    exd = torch.tensor(ex, dtype=torch.int64) if ex is not None else None
    idx, dist, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], exclude=exd)
    assert np.array_equal(r["idx"], _np(idx)) and np.array_equal(r["dist"], _np(dist))
    m = _marginal(F, X[rows], K, exclude=ex, G=G)
    assert np.array_equal(r["grid"], m["grid"]) and np.array_equal(r["bw"], m["bw"])
    assert r["dens"].shape == (B, len(r["pairs"]), G, G) and len(r["pairs"]) == (P * (P - 1) // 2 if pairs is None else len(pairs))
    _check_all(Y[r["idx"]].reshape(B, K, P), None, r, G)
    print("worst relative density error so far", WORST["rel"])


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("N,M,P,K,B,G,excl,pairs", [
    (2000, 6, 3, 257, 3, 64, True, None),
    (800, 5, 4, 1, 3, 17, True, None),                          # K = 1: the rectangular fallback
    (3000, 6, 2, 1025, 2, 65, False, [(1, 0)]),
])
def test_loclinear_against_adjusted_rows(ctx, kernel, N, M, P, K, B, G, excl, pairs):
    """Epanechnikov: unequal weights and the weight-0 last row; rectangular"""
    import torch
    from abcsmc_amd import device
    X, Y = _wl(M, P, N, 7 * N + K)
    F = _fit(ctx, X, Y, min(M, P))
    rows = np.arange(B) * 5
    ex = rows if excl else None
    a = device.rank_targets_adjust(F["Xd"], F["model"], F["A"], device.colmajor(X[rows], DEV), K, F["Yd"],
                                   exclude=torch.tensor(rows) if excl else None, kernel=kernel)
    torch.cuda.synchronize()
    a = _host(a)
    r = _joint(F, X[rows], K, exclude=ex, G=G, pairs=pairs, method=1, kernel=kernel, dist=True,
               adjust=("theta", "weight", "coef", "rank", "status"))
    for k in ("idx", "dist", "theta", "weight", "coef", "rank", "status"):
        assert np.array_equal(r[k], a[k]), k
    if kernel == 0 and K > 1:
        assert np.all(a["weight"][:, -1] == 0) and np.all(a["weight"][:, 0] > 0)
    m = _marginal(F, X[rows], K, exclude=ex, G=G, method=1, kernel=kernel)
    assert np.array_equal(r["grid"], m["grid"]) and np.array_equal(r["bw"], m["bw"])
    _check_all(a["theta"], a["weight"], r, G)
    print("worst relative density error so far", WORST["rel"])


def _generic(ctx, V, w=None, **kw):
    from abcsmc_amd import abcutil
    r = abcutil.weighted_joint(V, w, ctx=ctx, **kw)
    return {k: (v[None] if k in NAMES else v) for k, v in r.items()}


def test_generic_weights_pairs_and_given_bandwidths(ctx):
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(11)
    K, P, G = 700, 3, 65
    V = (rng.normal(size=(K, P)) @ np.array([[1.0, 0.5, 0.0], [0.0, 1.0, -0.7], [0.0, 0.0, 1.0]])) * np.array([1.0, 30.0, 1e-3])
    V += np.array([0.0, -200.0, 5.0])
    w = rng.uniform(0, 1, size=K)
    w[::7] = 0.0
    w[0] = 0.0                                                  # the first positive weight is not entry 0
    r = _generic(ctx, V, w, G=G)
    _check_all(V[None], w[None], r, G)
    m = abcutil.weighted_density(V, w, G=G, ctx=ctx)
    assert np.array_equal(r["grid"][0], m["grid"]) and np.array_equal(r["bw"][0], m["bw"])
    assert np.allclose(r["cov"][0], np.cov(V.T, aweights=w), rtol=1e-9, atol=0)
    # (j, i) as well as (i, j): the transpose within the same bound (both are within it of the same reference)
    t = _generic(ctx, V, w, G=G, pairs=[(0, 2), (2, 0), (1, 0)])
    _check_all(V[None], w[None], t, G)
    x0, x2 = D.grid_points(*t["grid"][0][0], G), D.grid_points(*t["grid"][0][2], G)
    f_ref = J.pair_density_at(V[:, 0], V[:, 2], w, x0, x2, t["bw"][0][0], t["bw"][0][2])
    assert np.all(np.abs(t["dens"][0][1].T.astype(LD) - f_ref) <= J.density_bound(f_ref))
    assert np.array_equal(t["dens"][0][0], r["dens"][0][1])      # the pair (0, 2) alone in another list: the same bits
    # options, and given bandwidths (bw_scale is not applied to them)
    o = _generic(ctx, V, w, G=17, bw_scale=0.37, cut=0.0)
    _check_all(V[None], w[None], o, 17)
    m = abcutil.weighted_density(V, w, G=17, bw_scale=0.37, cut=0.0, ctx=ctx)
    assert np.array_equal(o["grid"][0], m["grid"]) and np.array_equal(o["bw"][0], m["bw"])
    bw = np.array([0.5, 11.0, 2e-4])
    g = _generic(ctx, V, w, G=16, bw=bw, bw_scale=5.0)
    _check_all(V[None], w[None], g, 16, bw=bw[None])
    m = abcutil.weighted_density(V, w, G=16, bw=bw, bw_scale=5.0, ctx=ctx)
    assert np.array_equal(g["grid"][0], m["grid"]) and np.array_equal(g["bw"][0], m["bw"])
    print("worst relative density error so far", WORST["rel"])


def test_constant_offset_and_single_entries(ctx):
    rng = np.random.default_rng(12)
    K, G = 600, 33
    const = np.full(K, -2.5)                                    # variance exactly 0: no correlation with anything
    offset = 1e6 + rng.normal(size=K)                           # a one-pass covariance would lose the spread
    near = offset - 1e6 + 0.3 * rng.normal(size=K)
    V = np.stack([const, offset, near], axis=1)
    r = _generic(ctx, V, G=G)
    _check_all(V[None], None, r, G)
    c = r["corr"][0]
    assert np.isnan(c[0]).all() and np.isnan(c[:, 0]).all() and c[1, 1] == 1.0 and c[2, 2] == 1.0 and 0.9 < c[1, 2] < 1.0
    assert np.all(r["cov"][0][0] == 0.0)
    assert np.allclose(r["cov"][0][1:, 1:], np.cov(V[:, 1:].T), rtol=1e-9, atol=0)
    one = _generic(ctx, np.array([[3.0, 0.0, -1.0]]), G=15)     # K = 1: cov is 0 everywhere, the density one product kernel
    _check_all(np.array([[[3.0, 0.0, -1.0]]]), None, one, 15)
    assert np.all(one["cov"] == 0.0) and np.isnan(one["corr"]).all() and np.array_equal(one["mean"][0], [3.0, 0.0, -1.0])
    w = np.zeros(K)
    w[17] = 2.0                                                 # one entry with positive weight
    s = _generic(ctx, V, w, G=15)
    _check_all(V[None], w[None], s, 15)
    assert np.all(s["cov"] == 0.0) and np.array_equal(s["mean"][0], V[17])
    # two equal peaks on grid points: the smaller flat index is the mode
    two = np.array([[-1.0, -1.0], [1.0, 1.0]])
    t = _generic(ctx, two, G=65, cut=0.0, bw=0.3)
    assert tuple(t["mode"][0][0]) == (-1.0, -1.0) and t["mode_dens"][0][0] == t["dens"][0][0][0, 0]


def test_nan_and_inf_parameters(ctx):
    X, Y = _wl(5, 4, 1500, 3)
    Y = Y.copy()
    Y[::10, 1] = np.nan
    F = _fit(ctx, X, np.nan_to_num(Y, nan=0.0), 4)
    from abcsmc_amd import device
    F["Yd"] = device.colmajor(Y, DEV)
    rows = np.arange(4) * 9
    r = _joint(F, X[rows], 200, exclude=rows, G=17, pairs=[(0, 1), (0, 2), (1, 3), (3, 2), (2, 1)])
    vals = Y[r["idx"]]
    bad = ~np.isfinite(vals).all(axis=1)                        # (B, P)
    assert bad[:, 1].all() and not bad[:, [0, 2, 3]].any()
    with_bad = np.array([True, False, True, False, True])
    assert np.array_equal(np.isnan(r["dens"]).all(axis=(2, 3)), np.broadcast_to(with_bad, (4, 5)))
    assert np.array_equal(np.isnan(r["dens"]).any(axis=(2, 3)), np.broadcast_to(with_bad, (4, 5)))
    assert np.array_equal(np.isnan(r["mode_dens"]), np.broadcast_to(with_bad, (4, 5)))
    _check_all(vals, None, r, 17)
    # the others are unaffected: the same bits as without the bad parameter's column in the request
    F2 = dict(F, Yd=device.colmajor(np.nan_to_num(Y, nan=0.0), DEV))
    g = _joint(F2, X[rows], 200, exclude=rows, G=17, pairs=[(0, 2), (3, 2)])
    assert np.array_equal(g["idx"], r["idx"])
    assert np.array_equal(g["dens"], r["dens"][:, [1, 3]]) and np.array_equal(g["mode"], r["mode"][:, [1, 3]])
    keep = [0, 2, 3]
    assert np.array_equal(g["cov"][:, keep][:, :, keep], r["cov"][:, keep][:, :, keep])
    assert np.array_equal(g["mean"][:, keep], r["mean"][:, keep])
    V = np.random.default_rng(5).normal(size=(50, 2))
    V[3, 0] = np.inf
    i = _generic(ctx, V, np.where(np.arange(50) == 3, 0.0, 1.0), G=5)      # non-finite even under a zero weight
    assert np.isnan(i["dens"]).all() and np.isnan(i["mean"][0][0]) and np.isfinite(i["mean"][0][1])
    _check_all(V[None], np.where(np.arange(50) == 3, 0.0, 1.0)[None], i, 5)


def test_invariance(ctx):
    import torch
    from abcsmc_amd import abcutil, device
    X, Y = _wl(6, 4, 3000, 21)
    B, K, G = 20, 300, 65
    rows = np.arange(B) * 13
    for method in ("rejection", "loclinear"):
        kw = dict(method=method, exclude=rows, G=G, ctx=ctx)
        full = abcutil.particle_ranking_PLS_targets_joint(X, Y, X[rows], 0.5, K, **kw)
        assert full["dens"].shape == (B, 6, G, G) and full["x"].shape == (B, 4, G)
        for b in (0, 7, 19):                                    # alone and inside the batch
            one = abcutil.particle_ranking_PLS_targets_joint(X, Y, X[rows[b:b + 1]], 0.5, K, **dict(kw, exclude=rows[b:b + 1]))
            for k in NAMES:
                assert np.array_equal(one[k][0], full[k][b], equal_nan=True), (method, b, k)
        again = abcutil.particle_ranking_PLS_targets_joint(X, Y, X[rows], 0.5, K, **kw)
        for k in NAMES + ("idx", "dist"):
            assert np.array_equal(again[k], full[k], equal_nan=True), (method, k)
        nod = abcutil.particle_ranking_PLS_targets_joint(X, Y, X[rows], 0.5, K, dens=False, **kw)
        assert nod["dens"] is None
        for k in NAMES[:3] + NAMES[4:]:                         # nothing depends on dens being written
            assert np.array_equal(nod[k], full[k], equal_nan=True), (method, k)
        # a pair alone against the same pair among all pairs
        alone = abcutil.particle_ranking_PLS_targets_joint(X, Y, X[rows], 0.5, K, pairs=[(1, 3)], **kw)
        at = [tuple(p) for p in full["pairs"]].index((1, 3))
        for k in ("dens", "mode", "mode_dens"):
            assert np.array_equal(alone[k][:, 0], full[k][:, at]), (method, k)
        # the device entry with the same fit: the same bits, and idx / dist / adj those of the plain calls
        F = _fit(ctx, X, Y, 4)
        m = 0 if method == "rejection" else 1
        dev = _joint(F, X[rows], K, exclude=rows, G=G, method=m, dist=True, adjust=("theta", "weight") if m else ())
        assert np.array_equal(dev["idx"], full["idx"].astype(np.int64)) and np.array_equal(dev["dist"], full["dist"])
        for k in NAMES:
            assert np.array_equal(dev[k], full[k], equal_nan=True), (method, k)
        nod = _joint(F, X[rows], K, exclude=rows, G=G, method=m, dens=False)
        assert np.array_equal(nod["mode"], full["mode"]) and np.array_equal(nod["mode_dens"], full["mode_dens"])
        Td, exd = device.colmajor(X[rows], DEV), torch.tensor(rows)
        if m:
            a = _host(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], exclude=exd))
            for k in ("idx", "dist", "theta", "weight"):
                assert np.array_equal(dev[k], a[k]), k
        else:
            idx, dist, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], exclude=exd)
            assert np.array_equal(dev["idx"], _np(idx)) and np.array_equal(dev["dist"], _np(dist))
    # the generic entry: device and host
    rng = np.random.default_rng(2)
    V = rng.normal(size=(1500, 3))
    w = rng.uniform(0, 1, size=1500)
    h = abcutil.weighted_joint(V, w, G=17, ctx=ctx)
    d = _host(device.weighted_joint(torch.tensor(V.T.copy(), device=DEV), torch.tensor(w), G=17))
    for k in NAMES:
        assert np.array_equal(d[k], h[k]), k
    assert np.array_equal(d["pairs"], h["pairs"]) and np.array_equal(h["pairs"], [[0, 1], [0, 2], [1, 2]])


def test_argument_errors(ctx):
    import torch
    from abcsmc_amd import _lib, abcutil, device
    X, Y = _wl(5, 3, 800, 4)
    F = _fit(ctx, X, Y, 3)
    T = X[:4]
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -4
    N, M, P = 800, 5, 3
    Xf, Yf, Tf = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(T)
    hp = lambda v: v.ctypes.data_as(C.c_void_p) if v is not None else None
    dp = lambda t: t.data_ptr() if t is not None else None
    Td = device.colmajor(T, DEV)
    hmean, dmean = np.empty(4 * P), torch.empty(4 * P, dtype=torch.float64, device=DEV)
    hmd, dmd = np.empty(4 * 6), torch.empty(4 * 6, dtype=torch.float64, device=DEV)
    hbw, dbw = np.ones(4 * P), torch.ones(4 * P, dtype=torch.float64, device=DEV)

    def pr(*rows):
        return np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 2))

    def jt(mean, G=16, cut=3.0, bw_scale=1.0, bw=None, pairs=None, npairs=None, mode_dens=None):
        n = (0 if pairs is None else len(pairs)) if npairs is None else npairs
        return _lib.Joint(G, cut, bw_scale, bw, hp(pairs), n, mean, None, None, None, None, None, None, mode_dens)

    def host(B=4, K=50, Xm=Xf, Ym=Yf, Pm=P, mc=3, method=0, kernel=0, j=None):
        return L.abc_particle_ranking_pls_targets_joint(ctx.handle, hp(Xm), hp(Ym), N, M, Pm, hp(Tf), B, 0.5, mc, 0, None, K, method,
                                                        kernel, None, None, None, C.byref(j) if j is not None else None, None)

    def dev(B=4, K=50, Xm=F["Xd"], Ym=F["Yd"], Pm=P, md=F["model"], A=3, method=0, kernel=0, j=None):
        return L.abc_rank_targets_joint_dev(ctx.handle, dp(Xm), N, dp(Ym), N, N, M, Pm, dp(md), A, dp(Td), 4, B, None, K, method,
                                            kernel, None, None, None, C.byref(j) if j is not None else None)

    def refused(rc, code):
        assert rc == code, rc
        assert L.abc_last_error(ctx.handle)

    for call, mean, md, bwbuf, mk in ((host, hp(hmean), hp(hmd), hbw, hp), (dev, dmean.data_ptr(), dmd.data_ptr(), dbw, dp)):
        keep = [pr((0, 1), (3, 0)), pr((0, 1), (1, 1)), pr((-1, 2)), pr((2, 0), (0, 2), (1, 3)), pr((0, 1))]     # (kept alive)
        both, self_pair = pr((2, 0), (0, 2), (1, 2), (1, 2)), pr((0, 0))
        for bad in (dict(j=None), dict(j=jt(mean, G=1)), dict(j=jt(mean, G=0)), dict(j=jt(mean, G=257)),
                    dict(j=jt(mean, cut=-1.0)), dict(j=jt(mean, cut=np.nan)), dict(j=jt(mean, cut=np.inf)),
                    dict(j=jt(mean, bw_scale=0.0)), dict(j=jt(mean, bw_scale=-2.0)), dict(j=jt(mean, bw_scale=np.nan)),
                    dict(j=jt(mean, bw_scale=np.inf)), dict(j=jt(None)),
                    dict(j=jt(mean, pairs=keep[0])), dict(j=jt(mean, pairs=keep[1])), dict(j=jt(mean, pairs=keep[2])),
                    dict(j=jt(mean, pairs=keep[3])), dict(j=jt(mean, pairs=keep[4], npairs=0)),
                    dict(j=jt(mean), B=0), dict(j=jt(mean), K=0), dict(j=jt(mean), K=N + 1), dict(j=jt(mean), Xm=None),
                    dict(j=jt(mean), Ym=None), dict(j=jt(mean), method=2), dict(j=jt(mean), method=-1), dict(j=jt(mean), kernel=2)):
            refused(call(**bad), INVALID)
        refused(call(j=jt(mean), **{"mc" if call is host else "A": 65}), UNSUPPORTED)
        refused(call(j=jt(mean, pairs=keep[4], npairs=2 ** 22 + 1)), UNSUPPORTED)     # (refused before the list is read)
        for v in (0.0, -1.0, np.nan, np.inf):                   # a given bandwidth, checked on the device
            bwbuf[5] = v
            refused(call(j=jt(mean, bw=mk(bwbuf))), INVALID)
        bwbuf[5] = 1.0
        assert call(j=jt(mean, bw=mk(bwbuf))) == 0
        assert call(j=jt(mean, G=2)) == 0 and call(j=jt(mean, G=256, cut=0.0)) == 0
        assert call(j=jt(None, pairs=both, mode_dens=md)) == 0      # repeats and both orders are fine
        # P = 1 with pairs NULL: no pairs, the moments are written; a pair list cannot name anything
        if call is host:
            assert host(Ym=np.asfortranarray(Y[:, :1]), Pm=1, mc=1, j=jt(mean, mode_dens=md)) == 0
            refused(host(Ym=np.asfortranarray(Y[:, :1]), Pm=1, mc=1, j=jt(mean, pairs=self_pair)), INVALID)
    torch.cuda.synchronize()
    one = abcutil.particle_ranking_PLS_targets_joint(X, Y[:, :1], T, 0.5, 50, G=16, ctx=ctx)
    assert one["dens"].shape == (4, 0, 16, 16) and one["mode"].shape == (4, 0, 2) and one["cov"].shape == (4, 1, 1)
    assert np.all(np.isfinite(one["mean"])) and np.all(one["cov"] > 0) and np.all(one["corr"] == 1.0)
    # the generic entries: the densities' checks of V, ldv, K, P and the weights
    V = np.random.default_rng(0).normal(size=(100, 2))
    Vd = torch.tensor(V.T.copy(), device=DEV)
    for bad_w in (-np.ones(100), np.zeros(100), np.where(np.arange(100) == 7, np.nan, 1.0)):
        with pytest.raises(RuntimeError):
            abcutil.weighted_joint(V, bad_w, ctx=ctx)
        with pytest.raises(RuntimeError):
            device.weighted_joint(Vd, torch.tensor(bad_w))
    j = jt(dmean.data_ptr())
    for args in ((Vd.data_ptr(), 100, 0, 2), (Vd.data_ptr(), 100, 100, 0), (Vd.data_ptr(), 99, 100, 2), (None, 100, 100, 2)):
        refused(L.abc_weighted_joint_dev(ctx.handle, *args, None, C.byref(j)), INVALID)
    refused(L.abc_weighted_joint_dev(ctx.handle, Vd.data_ptr(), 100, 100, 2, None, None), INVALID)
    refused(L.abc_weighted_joint_dev(ctx.handle, Vd.data_ptr(), 100, 100, 2, None, C.byref(jt(dmean.data_ptr(), G=300))), INVALID)
    refused(L.abc_weighted_joint(ctx.handle, hp(np.asfortranarray(V)), 100, 2, None, C.byref(jt(None))), INVALID)
    for kw in (dict(bw=-1.0), dict(bw=[1.0, np.nan]), dict(G=257), dict(cut=-0.5), dict(bw_scale=0.0), dict(pairs=[(0, 2)]),
               dict(pairs=[(1, 1)])):
        with pytest.raises(RuntimeError):
            abcutil.weighted_joint(V, ctx=ctx, **kw)
    w1 = abcutil.weighted_joint(V[:, 0], ctx=ctx, G=8)          # one column: valid, no pairs
    assert w1["dens"].shape == (0, 8, 8) and w1["cov"].shape == (1, 1) and w1["cov"][0, 0] == pytest.approx(np.var(V[:, 0], ddof=1))
    # the context still works after the errors
    r = _generic(ctx, V, G=15)
    _check_all(V[None], None, r, 15)
