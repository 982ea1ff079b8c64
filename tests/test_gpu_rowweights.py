"""Row importance weights of the batched ranking (abc_ctx_set_row_weights, abc_ctx_set_row_weights_dev, abc_row_weights_info):
the ranking does not move; unit weights give the bits of the unset call through the RW kernel instances; the adjustment, alone,
under the variance correction, under ridge, under both and on a path, against the wrapped NumPy references (_rowweights_ref);
the weighted rejection means against a long-double mean; the products under method 0 against the generic entries on the retained
rows, bit for bit; the path summary under method 0 against the summary call at every tolerance; a target's bits alone, in a
batch, through the host entry and through strided views; the all-zero rule; the refusals; and the bias example end to end.

The setting lives in the context the whole suite shares, so every test sets it inside Context.row_weights(...), which restores
what was there before."""
import ctypes as C

import numpy as np
import pytest

import _rowweights_ref as RW
import _loclinear_ref as R
from test_gpu_hcorr import _fit, _np, _same, hetero_data

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1
L5 = (0.0, 1e-2, 1e-1, 1.0, 10.0)
PATTERNS = ("uniform", "lognormal", "zeros")

# (N, M, P, K, B, comps): direct gather, one chunk; the row-major table (4 B K >= N), chunks of 129 rows = a full tile of 128 and
# a tail of 1; seventeen chunks and the summaries' LDS path; more than 256 entry groups (the running sums pass through the
# workspace); the summaries' global sort path (method 0 only)
S_DIRECT, S_TABLE, S_CHUNKS, S_WIDE, S_GLOBAL = ((800, 5, 4, 16, 4, 0), (600, 5, 4, 257, 3, 0), (5000, 8, 6, 4097, 3, 0),
                                                 (1500, 16, 80, 300, 3, 12), (20000, 4, 2, 8193, 2, 0))
FIT_SHAPES = [S_DIRECT, S_TABLE, S_CHUNKS, S_WIDE]


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def omegas(N, pattern, seed):
    """the issue's weight patterns: uniform on (0.1, 2); exp of a normal with standard deviation 2; 30 % zeros"""
    rng = np.random.default_rng(1000 + seed)
    if pattern == "uniform":
        return rng.uniform(0.1, 2.0, N)
    if pattern == "lognormal":
        return np.exp(2.0 * rng.standard_normal(N))
    w = rng.uniform(0.1, 2.0, N)
    w[rng.uniform(size=N) < 0.3] = 0.0
    return w


_SETUPS = {}


def _setup(ctx, shape):
    """data, fit, targets of a shape, made once and shared (read only)"""
    if shape not in _SETUPS:
        from test_gpu_adjust import _with_nc
        N, M, P, K, B, comps = shape
        X, Y = hetero_data(N, M, P, 3 * N + K)
        A = comps if comps else min(M, P)
        F = _fit(ctx, X, Y, A)
        nc = comps if comps else F["ncomp"]
        rows = (np.arange(B) * 3) % N
        _SETUPS[shape] = (F, _with_nc(F, nc), nc, rows, np.ascontiguousarray(X[rows]))
    return _SETUPS[shape]


def _zeros_hit_a_first_row(ctx, shape, om):
    """the zeros pattern with the first retained row of target 0 among the zeros (the shift row has weight 0)"""
    F, model, nc, rows, T = _setup(ctx, shape)
    g = _adjust(ctx, F, model, T, shape[3], None, exclude=rows)
    om = om.copy()
    om[int(g["idx"][0, 0])] = 0.0
    return om


def _adjust(ctx, F, model, T, K, om, exclude=None, kernel=0, lam=None, hcorr=False, Y=None, X=None, **kw):
    """device.rank_targets_adjust under the row weights om (None: off), the ridge list lam and the variance correction"""
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(T, DEV) if isinstance(T, np.ndarray) else T
    ex = torch.tensor(np.asarray(exclude)) if exclude is not None else None
    with ctx.row_weights(om), ctx.adjust_ridge(lam), ctx.adjust_hcorr(hcorr):
        g = _np(device.rank_targets_adjust(F["Xd"] if X is None else X, model, F["A"], Td, K, F["Yd"] if Y is None else Y,
                                           exclude=ex, kernel=kernel, ctx=ctx, **kw))
        if lam is not None:
            g["pick"], g["press"] = ctx.last_ridge()
        if hcorr:
            g["hcoef"] = ctx.last_hcorr()
    return g


def _bound(g, ref, pert, keys, span, ok, tag):
    """the bound of test_gpu_hcorr.py / test_gpu_ridge.py, copied: 1e-9 of the parameter's range plus 100 x the reference's
    sensitivity to a relative 1e-15 perturbation of the scores, that widening below 1e-8 of the range"""
    for key in keys:
        sens = np.abs(pert[key] - ref[key]).max(axis=0)[ok]
        err = np.abs(g[key] - ref[key]).max(axis=0)[ok]
        if ok.any():
            print("%s %s: err/range %.3g, widening/range %.3g" % (tag, key, (err / span[ok]).max(), (100.0 * sens / span[ok]).max()))
        assert np.all(100.0 * sens < 1e-8 * span[ok]), (tag, key, "the case breaks the condition: other data, not a wider bound")
        assert np.all(err <= 1e-9 * span[ok] + 100.0 * sens), (tag, key, (err / span[ok]).max())


def _check_ref(F, T, g, b, nc, kernel, om, tag, lam=None, hcorr=False):
    """target b of an adjust call against the wrapped references; weight, rank and status exactly"""
    X, Y = F["X"], F["Y"]
    idx = g["idx"][b].astype(np.int64)
    S = R.scores(X[idx], F["mean"], F["sd"], F["R"], nc)
    o = R.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
    Sp = S * (1.0 + 1e-15 * np.random.default_rng(b).standard_normal(S.shape))

    def fit(Sx):
        if hcorr:
            return RW.hcorr(g["dist"][b], Sx, o, Y[idx], om[idx], kernel=kernel, A=F["A"], lambdas=lam)
        if lam is not None:
            return RW.ridge(g["dist"][b], Sx, o, Y[idx], om[idx], lam, kernel=kernel, A=F["A"])
        return RW.loclinear(g["dist"][b], Sx, o, Y[idx], om[idx], kernel=kernel, A=F["A"])
    ref, pert = fit(S), fit(Sp)
    span = Y.max(axis=0) - Y.min(axis=0)
    assert g["rank"][b] == ref["rank"] == pert["rank"] and g["status"][b] == ref["status"], (tag, b)
    assert _same(g["weight"][b], ref["weight"]), (tag, b)
    ok = np.ones(Y.shape[1], dtype=bool)
    left = 0
    if lam is not None:
        sure = (ref["gap"] > 1e-6) & (ref["pick"] == pert["pick"])
        assert np.array_equal(g["pick"][b][sure], ref["pick"][sure]), (tag, b, g["pick"][b], ref["pick"], ref["gap"])
        ok = sure & (g["pick"][b] == ref["pick"])
        left = int((~sure).sum())
        fin = np.isfinite(ref["press"])
        assert np.array_equal(np.isfinite(g["press"][b]), fin) and np.array_equal(np.isfinite(pert["press"]), fin), (tag, b)
        sens = np.abs(pert["press"][fin] - ref["press"][fin])
        err = np.abs(g["press"][b][fin] - ref["press"][fin])
        assert np.all(100.0 * sens < 1e-8 * ref["press"][fin]), (tag, b, "press", "the case breaks the condition")
        assert np.all(err <= 1e-9 * ref["press"][fin] + 100.0 * sens), (tag, b, "press", (err / ref["press"][fin]).max())
    if hcorr:
        assert np.array_equal(np.isnan(g["hcoef"][b][0]), ref["skipped"]), (tag, b)
        ok = ok & ~ref["skipped"]
    gb = {k: g[k][b] for k in ("coef", "theta") + (("hcoef",) if hcorr else ())}
    _bound(gb, ref, pert, tuple(gb), span, ok, "%s b=%d" % (tag, b))
    assert np.all(g["coef"][b][1 + nc:] == 0.0)
    return left


# ---- the ranking and the rejection means ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [S_DIRECT, S_TABLE, S_CHUNKS, S_WIDE, S_GLOBAL])
def test_ranking_does_not_move_and_rejection_mean(ctx, shape):
    """idx and dist with `exclude` are the unset call's bits under every weight pattern; post_mean is the weighted mean within
    1e-9 of the parameter's range (the project's bound for its fp64 stages); unit weights give the unset post_mean's bits"""
    import torch
    from abcsmc_amd import device
    N, M, P, K, B, _ = shape
    F, model, nc, rows, T = _setup(ctx, shape)
    Td, ex = device.colmajor(T, DEV), torch.tensor(rows)
    span = F["Y"].max(axis=0) - F["Y"].min(axis=0)

    def call():
        idx, dist, pm = device.rank_targets(F["Xd"], model, F["A"], Td, K, Y=F["Yd"], exclude=ex, post_mean=True, ctx=ctx)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dist.cpu().numpy(), pm.cpu().numpy()
    idx0, dist0, pm0 = call()
    with ctx.row_weights(np.ones(N)):
        idx1, dist1, pm1 = call()
    assert _same(idx0, idx1) and _same(dist0, dist1) and _same(pm0, pm1)
    for pattern in PATTERNS:
        om = omegas(N, pattern, K)
        with ctx.row_weights(om):
            idx, dist, pm = call()
        assert _same(idx, idx0) and _same(dist, dist0), pattern
        for b in range(B):
            ref = RW.post_mean(F["Y"][idx[b]], om[idx[b]])
            err = np.abs(pm[b].astype(np.longdouble) - ref).astype(np.float64)
            print("post_mean", shape, pattern, b, "err/range %.3g" % (err / span).max())
            assert np.all(err <= 1e-9 * span), (shape, pattern, b, (err / span).max())
        assert not _same(pm, pm0)
    idx2, dist2, pm2 = call()                                       # cleared: the unset bits
    assert _same(idx0, idx2) and _same(pm0, pm2)


# ---- unit weights: other instances, the same arithmetic --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_unit_weights_give_the_unset_bits(ctx, shape):
    import torch
    from abcsmc_amd import device
    N, M, P, K, B, _ = shape
    F, model, nc, rows, T = _setup(ctx, shape)
    one = np.ones(N)
    for kernel in (0, 1):
        for lam, hc in ((None, False), (None, True), (L5, False), (L5, True)):
            off = _adjust(ctx, F, model, T, K, None, exclude=rows, kernel=kernel, lam=lam, hcorr=hc)
            on = _adjust(ctx, F, model, T, K, one, exclude=rows, kernel=kernel, lam=lam, hcorr=hc)
            assert set(off) == set(on)
            for k in off:
                assert _same(off[k], on[k]), (shape, kernel, lam, hc, k)
    Td, ex = device.colmajor(T, DEV), torch.tensor(rows)
    Ks = (3, max(4, K // 3), K)
    args = (F["Xd"], model, F["A"], Td)

    def calls():
        r = {"path": device.rank_targets_path(*args, Ks, F["Yd"], exclude=ex, ctx=ctx)}
        r["summary"] = device.rank_targets_summary(*args, K, F["Yd"], truth=torch.tensor(F["Y"][rows]), method=1, exclude=ex, ctx=ctx)
        r["density"] = device.rank_targets_density(*args, K, F["Yd"], G=65, method=1, exclude=ex, ctx=ctx)
        r["joint"] = device.rank_targets_joint(*args, K, F["Yd"], G=16, pairs=[(0, 1)], method=1, exclude=ex, ctx=ctx)
        r["draws"] = device.rank_targets_draws(*args, K, F["Yd"], 129, smooth=True, seed=5, method=1, exclude=ex, ctx=ctx)
        r["path_summary"] = device.rank_targets_path_summary(*args, Ks, F["Yd"], method=1, exclude=ex, ctx=ctx)
        return {k: _np(v) for k, v in r.items()}
    before = calls()
    with ctx.row_weights(one):
        during = calls()
    for name in before:
        for k in before[name]:
            if isinstance(before[name][k], np.ndarray):
                assert _same(before[name][k], during[name][k]), (shape, name, k)


# ---- against the reference --------------------------------------------------------------------------------------------------------
# The seed of the weights per (shape, pattern): K unless named here.  The bound carries its own condition (100 x the reference's
# sensitivity to a relative 1e-15 perturbation of the scores stays below 1e-8 of the range), which is a property of the data; the
# second fit of the variance correction regresses log residuals and is the touchy one where the weights leave few effective rows
# per coefficient.  Worked out on the references alone, on this file's own tables with the scores of a NumPy PLS fit (_pls_ref;
# it reproduces the widenings the device run prints to two digits) and the rows ranked by their distance in score space, plain
# and L5, targets 0 and B - 1, worst widening over coef, theta and hcoef as a fraction of the range:
#   (800, 5, 4, 16), both kernels: lognormal 7e-12 and zeros 4e-11 at seed K = 16; seeds 16 to 35 range from 2e-12 to 4e-8
#   (1500, 16, 80, 300) nc = 12 lognormal (80 parameters, about 43 effective rows for 13 coefficients): seeds 300 to 335 range
#   from 1e-10 to 3e-8; seed K = 300 gives 2e-9, inside the condition with little room, seed 329 gives 1e-10 and is taken
WEIGHT_SEED = {(S_WIDE, "lognormal"): 329}
SETTINGS = ((None, False), (L5, False), (None, True), (L5, True))         # (ridge list, hcorr): every case checks all four


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_adjustment_against_reference(ctx, shape, pattern):
    """the adjustment alone, under hcorr, under ridge and under both, against the wrapped references"""
    N, M, P, K, B, _ = shape
    F, model, nc, rows, T = _setup(ctx, shape)
    om = omegas(N, pattern, WEIGHT_SEED.get((shape, pattern), K))
    if pattern == "zeros":
        om = _zeros_hit_a_first_row(ctx, shape, om)
    off = _adjust(ctx, F, model, T, K, None, exclude=rows)
    left, pairs = 0, 0
    for kernel in ((0, 1) if shape == S_DIRECT else (0,)):
        for lam, hc in SETTINGS:
            g = _adjust(ctx, F, model, T, K, om, exclude=rows, kernel=kernel, lam=lam, hcorr=hc)
            if kernel == 0:
                assert _same(g["idx"], off["idx"]) and _same(g["dist"], off["dist"])
            for b in sorted({0, B - 1}):
                n = _check_ref(F, T, g, b, nc, kernel, om, (shape, pattern, kernel, lam is not None, hc), lam=lam, hcorr=hc)
                if lam is not None:
                    left, pairs = left + n, pairs + P
    assert 100 * left <= max(pairs, 100), (left, pairs)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_path_against_reference(ctx, pattern):
    """a path of three tolerances: coef, rank, status against the wrapped reference, post_mean against the long-double weighted
    mean, and slot (b, t) of coef within the same bound of the adjust call at K_t"""
    import torch
    from abcsmc_amd import device
    shape = S_TABLE
    N, M, P, K, B, _ = shape
    F, model, nc, rows, T = _setup(ctx, shape)
    om = omegas(N, pattern, K)
    if pattern == "zeros":
        om = _zeros_hit_a_first_row(ctx, shape, om)
    Ks = (nc + 1, 64, K)
    Td, ex = device.colmajor(T, DEV), torch.tensor(rows)
    with ctx.row_weights(om):
        g = _np(device.rank_targets_path(F["Xd"], model, F["A"], Td, Ks, F["Yd"], exclude=ex, ctx=ctx))
    span = F["Y"].max(axis=0) - F["Y"].min(axis=0)
    ok = np.ones(P, dtype=bool)
    for b in range(B):
        idx = g["idx"][b].astype(np.int64)
        S = R.scores(F["X"][idx], F["mean"], F["sd"], F["R"], nc)
        o = R.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
        Sp = S * (1.0 + 1e-15 * np.random.default_rng(b).standard_normal(S.shape))
        ref = RW.path(g["dist"][b], S, o, F["Y"][idx], om[idx], Ks, A=F["A"])
        pert = RW.path(g["dist"][b], Sp, o, F["Y"][idx], om[idx], Ks, A=F["A"])
        assert np.array_equal(g["rank"][b], ref["rank"]) and np.array_equal(g["status"][b], ref["status"]), (pattern, b)
        assert _same(g["h"][b], ref["h"])
        for t in range(len(Ks)):
            if t == 0 and not np.all(np.isfinite(ref["coef"][0])):
                continue
            _bound({"coef": g["coef"][b, t]}, {"coef": ref["coef"][t]}, {"coef": pert["coef"][t]}, ("coef",), span, ok,
                   "path %s b=%d t=%d" % (pattern, b, t))
        err = np.abs(g["post_mean"][b].astype(np.longdouble) - ref["post_mean"]).astype(np.float64)
        assert np.all(err <= 1e-9 * span), (pattern, b, (err / span).max())


# ---- the smallest retained counts -------------------------------------------------------------------------------------------------
def test_smallest_retained_counts(ctx):
    """K = 1, K = 2 and K = nc + 1 under every pattern: weight bit for bit, rank and status as the reference; coef against the
    reference where the sensitivity condition of the bound holds (with so few rows the fit interpolates or is rank deficient, and
    the pivots decide), the weighted post_mean always"""
    import torch
    from abcsmc_amd import device
    shape = S_DIRECT
    N, M, P, _, B, _ = shape
    F, model, nc, rows, T = _setup(ctx, shape)
    span = F["Y"].max(axis=0) - F["Y"].min(axis=0)
    Td, ex = device.colmajor(T, DEV), torch.tensor(rows)
    for K in (1, 2, nc + 1):
        for pattern in PATTERNS:
            om = omegas(N, pattern, K)
            g = _adjust(ctx, F, model, T, K, om, exclude=rows)
            with ctx.row_weights(om):
                pm = device.rank_targets(F["Xd"], model, F["A"], Td, K, Y=F["Yd"], exclude=ex, post_mean=True, ctx=ctx)[2].cpu().numpy()
            for b in range(B):
                idx = g["idx"][b].astype(np.int64)
                S = R.scores(F["X"][idx], F["mean"], F["sd"], F["R"], nc)
                o = R.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
                ref = RW.loclinear(g["dist"][b], S, o, F["Y"][idx], om[idx], A=F["A"])
                assert _same(g["weight"][b], ref["weight"]), (K, pattern, b)
                assert bool(g["status"][b] & 4) == (not np.any(ref["weight"] > 0)) == bool(ref["status"] & 4), (K, pattern, b)
                assert np.array_equal(np.isnan(g["coef"][b]), np.isnan(ref["coef"])), (K, pattern, b)
                pert = RW.loclinear(g["dist"][b], S * (1.0 + 1e-15 * np.random.default_rng(b).standard_normal(S.shape)), o,
                                    F["Y"][idx], om[idx], A=F["A"])
                with np.errstate(all="ignore"):
                    sens = np.abs(pert["coef"] - ref["coef"]).max(axis=0)
                    fine = (100.0 * sens < 1e-8 * span) & (ref["rank"] == pert["rank"])
                if ref["rank"] == pert["rank"]:                    # (the pivots are decided: rank and every status bit)
                    assert g["rank"][b] == ref["rank"] and g["status"][b] == ref["status"], (K, pattern, b, g["rank"][b],
                                                                                             g["status"][b], ref["rank"], ref["status"])
                if fine.any() and g["rank"][b] == ref["rank"]:
                    err = np.abs(g["coef"][b] - ref["coef"]).max(axis=0)
                    assert np.all(err[fine] <= 1e-9 * span[fine] + 100.0 * sens[fine]), (K, pattern, b)
                want = RW.post_mean(F["Y"][idx], om[idx])
                with np.errstate(all="ignore"):
                    e = np.abs(pm[b].astype(np.longdouble) - want).astype(np.float64)
                assert np.array_equal(np.isnan(pm[b]), np.isnan(want.astype(np.float64))) and np.all((e <= 1e-9 * span) | np.isnan(e))


# ---- the products under method 0: the generic entries on the retained rows --------------------------------------------------------
def _generic(ctx, F, om, idx_b, what, **kw):
    import torch
    from abcsmc_amd import device
    V = device.colmajor(np.ascontiguousarray(F["Y"][idx_b]), DEV)
    w = torch.tensor(om[idx_b], dtype=torch.float64, device=DEV)
    return _np(getattr(device, "weighted_" + what)(V, w, ctx=ctx, **kw))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", [S_DIRECT, S_CHUNKS, S_GLOBAL])
def test_rejection_products_are_the_generic_entries_on_the_retained_rows(ctx, shape, pattern):
    """summary, density, joint and draws (an explicit stream and seed) under method 0 with the weights: target b has the bits of
    the generic entry on V = Y[idx[b]] and w = omega[idx[b]]"""
    import torch
    from abcsmc_amd import device
    N, M, P, K, B, _ = shape
    F, model, nc, rows, T = _setup(ctx, shape)
    om = omegas(N, pattern, K + 1)
    Td, ex = device.colmajor(T, DEV), torch.tensor(rows)
    args = (F["Xd"], model, F["A"], Td, K, F["Yd"])
    truth = F["Y"][rows].copy()
    stream = [11 + 3 * b for b in range(B)]
    with ctx.row_weights(om):
        sm = _np(device.rank_targets_summary(*args, truth=torch.tensor(truth), exclude=ex, ctx=ctx))
        dn = _np(device.rank_targets_density(*args, G=65, exclude=ex, ctx=ctx))
        jt = _np(device.rank_targets_joint(*args, G=16, exclude=ex, ctx=ctx))
        dr = [_np(device.rank_targets_draws(*args, 257, smooth=s, seed=9, stream=stream, exclude=ex, ctx=ctx)) for s in (False, True)]
    unset = _np(device.rank_targets_summary(*args, truth=torch.tensor(truth), exclude=ex, ctx=ctx))
    assert _same(sm["idx"], unset["idx"]) and not _same(sm["quant"], unset["quant"])
    for b in range(B):
        ib = sm["idx"][b].astype(np.int64)
        assert np.any(om[ib] > 0)
        g = _generic(ctx, F, om, ib, "summary", truth=torch.tensor(truth[b]))
        assert _same(g["quant"], sm["quant"][b]) and _same(g["cdf"], sm["cdf"][b]), (shape, pattern, b, "summary")
        g = _generic(ctx, F, om, ib, "density", G=65)
        for k in ("dens", "grid", "bw", "mode", "mode_dens"):
            assert _same(g[k], dn[k][b]), (shape, pattern, b, "density", k)
        g = _generic(ctx, F, om, ib, "joint", G=16)
        for k in ("mean", "cov", "corr", "dens", "grid", "bw", "mode", "mode_dens"):
            assert _same(g[k], jt[k][b]), (shape, pattern, b, "joint", k)
        for s, d in zip((False, True), dr):
            g = _generic(ctx, F, om, ib, "draws", S=257, smooth=s, seed=9, stream=stream[b])
            for k in ("draws", "src", "ess", "bw"):
                assert _same(g[k], d[k][b]), (shape, pattern, b, "draws", s, k)
            assert 0.0 < d["ess"][b] < K


@pytest.mark.parametrize("shape,Ks", [(S_TABLE, (3, 64, 257)), (S_GLOBAL, (100, 4097, 8193))])
def test_path_summary_under_rejection_is_the_summary_call_at_every_tolerance(ctx, shape, Ks):
    import torch
    from abcsmc_amd import device
    N, M, P, K, B, _ = shape
    F, model, nc, rows, T = _setup(ctx, shape)
    om = omegas(N, "zeros", K + 2)
    Td, ex = device.colmajor(T, DEV), torch.tensor(rows)
    truth = torch.tensor(F["Y"][rows])
    with ctx.row_weights(om):
        g = _np(device.rank_targets_path_summary(F["Xd"], model, F["A"], Td, Ks, F["Yd"], truth=truth, exclude=ex, ctx=ctx))
        for t, Kt in enumerate(Ks):
            s = _np(device.rank_targets_summary(F["Xd"], model, F["A"], Td, Kt, F["Yd"], truth=truth, exclude=ex, ctx=ctx))
            assert _same(g["quant"][:, t], s["quant"]) and _same(g["cdf"][:, t], s["cdf"]), (shape, Kt)
    plain = _np(device.rank_targets_path_summary(F["Xd"], model, F["A"], Td, Ks, F["Yd"], truth=truth, exclude=ex, ctx=ctx))
    assert _same(plain["idx"], g["idx"]) and not _same(plain["quant"], g["quant"])


# ---- the same bits ------------------------------------------------------------------------------------------------------------------
def test_alone_in_a_batch_through_the_host_entry_and_strided_views(ctx):
    import torch
    from abcsmc_amd import abcutil, device
    N, M, P, K, B = 3000, 6, 3, 200, 12
    X, Y = hetero_data(N, M, P, 5)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 7
    T = np.ascontiguousarray(X[rows])
    om = omegas(N, "zeros", 3)
    g = _adjust(ctx, F, F["model"], T, K, om, exclude=rows, lam=L5, hcorr=True)
    host = abcutil.particle_ranking_PLS_targets_adjust(X, Y, T, 0.5, K, exclude=rows, max_comp=3, rule=0, ctx=ctx, ridge=L5,
                                                       hcorr=True, row_weights=om)
    assert host["ncomp"] == F["ncomp"] and ctx._row_weights is None and ctx.row_weights_info()[0] == 0      # restored
    for k in ("idx", "theta", "weight", "coef", "rank", "status", "hcoef"):
        assert _same(host[k], g[k]), k
    assert _same(host["ridge_pick"], g["pick"]) and _same(host["ridge_press"], g["press"])
    for b in (0, 5, B - 1):
        one = _adjust(ctx, F, F["model"], T[b:b + 1], K, om, exclude=rows[b:b + 1], lam=L5, hcorr=True)
        for k in ("idx", "theta", "weight", "coef", "pick", "press", "hcoef"):
            assert _same(one[k][0], g[k][b]), (k, b)
    xbig = torch.full((M, N + 5), float("nan"), dtype=torch.float64, device=DEV)
    ybig = torch.full((P, N + 3), float("nan"), dtype=torch.float64, device=DEV)
    tbig = torch.full((M, B + 2), float("nan"), dtype=torch.float64, device=DEV)
    xbig[:, 1:N + 1], ybig[:, 2:N + 2], tbig[:, 1:B + 1] = F["Xd"], F["Yd"], device.colmajor(T, DEV)
    v = _adjust(ctx, F, F["model"], tbig[:, 1:B + 1], K, om, exclude=rows, lam=L5, hcorr=True, X=xbig[:, 1:N + 1], Y=ybig[:, 2:N + 2])
    for k in ("idx", "theta", "weight", "coef", "pick", "press", "hcoef"):
        assert _same(v[k], g[k]), k
    # device weights through abc_ctx_set_row_weights_dev: the same bits, and the caller's tensor may go away after the call
    omd = torch.tensor(om, device=DEV)
    with ctx.row_weights(omd):
        del omd
        d = _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"],
                                           exclude=torch.tensor(rows), ctx=ctx))
    p = _adjust(ctx, F, F["model"], T, K, om, exclude=rows)
    for k in ("theta", "weight", "coef"):
        assert _same(d[k], p[k]), k
    # the rejection mean and a product through the host entries
    with ctx.row_weights(om):
        pm = device.rank_targets(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, Y=F["Yd"], exclude=torch.tensor(rows),
                                 post_mean=True, ctx=ctx)[2].cpu().numpy()
        sm = _np(device.rank_targets_summary(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"],
                                             exclude=torch.tensor(rows), ctx=ctx))
    hp = abcutil.particle_ranking_PLS_targets(X, Y, T, 0.5, K, exclude=rows, max_comp=3, rule=0, details=True, ctx=ctx, row_weights=om)
    hs = abcutil.particle_ranking_PLS_targets_summary(X, Y, T, 0.5, K, exclude=rows, max_comp=3, rule=0, ctx=ctx, row_weights=om)
    assert _same(hp["post_mean"], pm) and _same(hs["quant"], sm["quant"])


# ---- the all-zero rule --------------------------------------------------------------------------------------------------------------
def test_a_target_whose_retained_rows_all_weigh_zero(ctx):
    import torch
    from abcsmc_amd import device
    N, M, P, K, B = 3000, 6, 3, 64, 4
    X, Y = hetero_data(N, M, P, 9)
    F = _fit(ctx, X, Y, 3)
    nc = F["ncomp"]
    rows = np.array([0, 700, 1500, 2400])
    T = np.ascontiguousarray(X[rows])
    plain = _adjust(ctx, F, F["model"], T, K, None, exclude=rows)
    om = omegas(N, "uniform", 4)
    z = 2
    om[plain["idx"][z].astype(np.int64)] = 0.0
    others = [b for b in range(B) if b != z]
    assert all(np.any(om[plain["idx"][b].astype(np.int64)] > 0) for b in others)
    ctx.adjust_hcorr_skipped(reset=True)
    ctx.adjust_ridge_unscored(reset=True)
    g = _adjust(ctx, F, F["model"], T, K, om, exclude=rows, lam=L5, hcorr=True)
    skipped, unscored = ctx.adjust_hcorr_skipped(reset=True), ctx.adjust_ridge_unscored(reset=True)
    rest = _adjust(ctx, F, F["model"], T[others], K, om, exclude=rows[others], lam=L5, hcorr=True)
    skipped_rest, unscored_rest = ctx.adjust_hcorr_skipped(reset=True), ctx.adjust_ridge_unscored(reset=True)
    assert skipped - skipped_rest == P and unscored - unscored_rest == P
    assert g["status"][z] & 4 and g["rank"][z] == 0 and g["status"][z] == (4 | (1 if nc else 0) | (plain["status"][z] & 2))
    assert not np.any(g["status"][others] & 4)
    assert np.all(np.isnan(g["coef"][z][:1 + nc])) and np.all(g["coef"][z][1 + nc:] == 0.0)
    assert np.all(np.isnan(g["theta"][z])) and np.all(g["weight"][z] == 0.0)
    assert np.all(np.isnan(g["hcoef"][z][0])) and np.all(g["hcoef"][z][1:] == 0.0)
    assert np.all(g["pick"][z] == len(L5) - 1) and np.all(g["press"][z] == np.inf)
    for k in ("idx", "dist", "theta", "weight", "coef", "rank", "status", "hcoef", "pick", "press"):
        assert _same(g[k][others], rest[k]), k
    alone = _adjust(ctx, F, F["model"], T, K, om, exclude=rows)           # without ridge and hcorr: k_adj_solve's own rule
    assert np.all(np.isnan(alone["coef"][z][:1 + nc])) and np.all(np.isnan(alone["theta"][z])) and alone["status"][z] & 4
    # without components (nc = 0) there is no slope to carry the NaN: the rows are NaN all the same, the others' rows their own
    from test_gpu_adjust import _with_nc
    m0 = _with_nc(F, 0)
    p0 = _adjust(ctx, F, m0, T, K, None, exclude=rows)                    # (nc = 0 ranks on nothing: its own retained rows)
    om0 = omegas(N, "uniform", 5)
    om0[p0["idx"][z].astype(np.int64)] = 0.0
    g0 = _adjust(ctx, F, m0, T, K, om0, exclude=rows)
    assert _same(g0["idx"], p0["idx"])
    zi = np.flatnonzero(np.all(om0[g0["idx"].astype(np.int64)] == 0.0, axis=1))
    assert z in zi
    for b in range(B):
        if b in zi:
            assert g0["status"][b] == (4 | (p0["status"][b] & 2)) and g0["rank"][b] == 0, b
            assert np.all(np.isnan(g0["coef"][b][0])) and np.all(g0["coef"][b][1:] == 0.0) and np.all(np.isnan(g0["theta"][b])), b
        else:
            assert not g0["status"][b] & 4 and np.array_equal(g0["theta"][b], Y[g0["idx"][b].astype(np.int64)]), b
    live = _adjust(ctx, F, m0, T, K, omegas(N, "uniform", 6), exclude=rows)    # positive weights: the rows unchanged, as without
    assert not np.any(live["status"] & 4) and np.array_equal(live["theta"], Y[live["idx"].astype(np.int64)])
    # the path: every tolerance of the target is an all-zero slot
    Td, ex = device.colmajor(T, DEV), torch.tensor(rows)
    with ctx.row_weights(om):
        p = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], Td, (8, K), F["Yd"], exclude=ex, ctx=ctx))
        po = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], device.colmajor(T[others], DEV), (8, K), F["Yd"],
                                          exclude=torch.tensor(rows[others]), ctx=ctx))
    assert np.all(p["status"][z] & 4) and np.all(p["rank"][z] == 0) and np.all(np.isnan(p["coef"][z][:, :1 + nc]))
    assert np.all(np.isnan(p["post_mean"][z]))
    for k in ("coef", "post_mean", "rank", "status", "h"):
        assert _same(p[k][others], po[k]), k
    # the products: NaN, ess 0, src 0 for the target, the others as in a batch without it; both methods
    for method in (0, 1):
        def products(Tx, rx):
            a = (F["Xd"], F["model"], F["A"], device.colmajor(Tx, DEV), K, F["Yd"])
            kw = dict(method=method, exclude=torch.tensor(rx), ctx=ctx)
            r = {"summary": device.rank_targets_summary(*a, truth=torch.tensor(Y[rx]), **kw)}
            r["density"] = device.rank_targets_density(*a, G=33, **kw)
            r["joint"] = device.rank_targets_joint(*a, G=8, **kw)
            r["draws"] = device.rank_targets_draws(*a, 70, seed=3, stream=[int(v) for v in rx], **kw)
            r["smooth"] = device.rank_targets_draws(*a, 70, smooth=True, seed=3, stream=[int(v) for v in rx], **kw)
            return {k: _np(v) for k, v in r.items()}
        with ctx.row_weights(om):
            full, part = products(T, rows), products(T[others], rows[others])
        for name in full:
            for k, v in full[name].items():
                if not isinstance(v, np.ndarray) or k in ("idx", "dist", "pairs"):
                    continue
                assert _same(v[others], part[name][k]), (method, name, k)
                if v.dtype.kind == "f" and k != "ess":
                    assert np.all(np.isnan(v[z])), (method, name, k)
        for name in ("draws", "smooth"):
            assert full[name]["ess"][z] == 0.0 and np.all(full[name]["src"][z] == 0), (method, name)


# ---- bad arguments ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_clearing():
    from abcsmc_amd import _lib, abcutil
    Lb = _lib.lib()
    c = _lib.Context(0)
    assert c.row_weights_info() == (0, 0, 0.0)
    X, Y = hetero_data(500, 4, 2, 1)
    kw = dict(max_comp=2, rule=0, ctx=c)
    unset = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)
    good = omegas(500, "zeros", 1)
    c.set_row_weights(good)
    n, pos, ess = c.row_weights_info()
    assert n == 500 and pos == int((good > 0).sum()) and abs(ess - good.sum() ** 2 / (good ** 2).sum()) <= 1e-12 * ess
    want = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)
    assert not _same(want["coef"], unset["coef"]) and _same(want["idx"], unset["idx"])
    bads = []
    for v in (-1.0, float("nan"), float("inf"), -float("inf")):
        b = good.copy()
        b[123] = v
        bads.append(b)
    bads.append(np.zeros(500))
    bads.append(np.full(500, 1e200))                                       # finite, but the sum of squares is not
    for b in bads:
        assert Lb.abc_ctx_set_row_weights(c.handle, b.ctypes.data, b.size) == INVALID
        assert b"row weights" in Lb.abc_last_error(c.handle)
        assert c.row_weights_info()[0] == 500                              # the previous setting is in force
        got = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)
        assert _same(got["coef"], want["coef"])
    # a call whose N differs from the stored count, through every kind of entry
    with pytest.raises(_lib.AbcError):
        abcutil.particle_ranking_PLS_targets_adjust(X[:400], Y[:400], X[:3], 0.5, 50, **kw)
    with pytest.raises(_lib.AbcError):
        abcutil.particle_ranking_PLS_targets(X[:400], Y[:400], X[:3], 0.5, 50, **kw)
    with pytest.raises(_lib.AbcError):
        abcutil.particle_ranking_PLS_targets_summary(X[:400], Y[:400], X[:3], 0.5, 50, **kw)
    with pytest.raises(_lib.AbcError):
        abcutil.particle_ranking_PLS_targets_path(X[:400], Y[:400], X[:3], 0.5, (5, 50), **kw)
    again = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)      # the context still works
    assert _same(again["coef"], want["coef"])
    c.set_row_weights(None)
    assert c.row_weights_info() == (0, 0, 0.0)
    off = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)
    for k in ("idx", "dist", "theta", "weight", "coef", "rank", "status"):
        assert _same(off[k], unset[k]), k
    abcutil.particle_ranking_PLS_targets_adjust(X[:400], Y[:400], X[:3], 0.5, 50, **kw)  # and any N is fine again
    assert Lb.abc_ctx_set_row_weights(c.handle, None, 5) == 0 and Lb.abc_ctx_set_row_weights(c.handle, good.ctypes.data, 0) == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_the_weights_remove_the_design_bias(ctx):
    """test_rowweights_cpu.py's example through abcutil.particle_ranking_PLS_targets with its seed: the mean bias of the
    weighted rejection mean over the targets is at most a quarter of the unweighted one"""
    from abcsmc_amd import abcutil
    from test_rowweights_cpu import BIAS_K, BIAS_SEED, bias_example
    e = bias_example(BIAS_SEED)
    kw = dict(max_comp=1, rule=0, details=True, ctx=ctx)
    prior = abcutil.particle_ranking_PLS_targets(e["X_prior"], e["theta_prior"][:, None], e["targets"], 0.5, BIAS_K, **kw)["post_mean"]
    unw = abcutil.particle_ranking_PLS_targets(e["X"], e["theta"][:, None], e["targets"], 0.5, BIAS_K, **kw)["post_mean"]
    wtd = abcutil.particle_ranking_PLS_targets(e["X"], e["theta"][:, None], e["targets"], 0.5, BIAS_K, row_weights=e["omega"],
                                               **kw)["post_mean"]
    bu, bw = abs(float((unw - prior).mean())), abs(float((wtd - prior).mean()))
    print("bias example (device): unweighted %.4f, weighted %.4f" % (bu, bw))
    assert bw <= 0.25 * bu, (bu, bw)


def test_weight_predictive_prior_output_is_accepted_as_is(ctx):
    """one real Generation step; its proposals simulated into a new table; weight_predictive_prior's output for all N rows of that
    table as the row weights: the call completes and reports a finite ess"""
    import torch
    from abcsmc_amd import _lib, abcutil, device, synthetic
    N, M, P, K, Kp, Nn, A = 4096, 8, 4, 256, 256, 2048, 4
    wl = synthetic.Workload(M, P)
    X, Y = wl.rows(0, N)
    spec = wl.prior_spec()
    th_prev, w_prev, dv_prev = wl.previous_set(Kp)
    gen = device.Generation(N, M, P, K, Kp, Nn, train_frac=0.5, max_comp=A, multivariate=True, device=DEV, ctx=ctx)
    gen.run(device.colmajor(X, DEV), device.colmajor(Y, DEV), device.colmajor(wl.observed(), DEV),
            device.priors_to_device(_lib.make_priors(spec), DEV), abcutil.rng(4242), device.colmajor(th_prev, DEV),
            device.colmajor(w_prev, DEV), device.colmajor(dv_prev, DEV))
    torch.cuda.synchronize()
    theta = np.ascontiguousarray(device.to_numpy(gen.next))               # (Nn, P): the next set's parameters
    assert theta.shape == (Nn, P) and np.all(np.isfinite(theta))
    sel, w_sel, dv = np.ascontiguousarray(device.to_numpy(gen.theta)), gen.w.cpu().numpy(), gen.dv.cpu().numpy()
    rng = np.random.default_rng(8)
    Xn = theta @ rng.normal(0.0, 1.0, (P, M)) + 0.3 * rng.standard_normal((Nn, M))
    om = abcutil.weight_predictive_prior(_lib.make_priors(spec), theta, sel, w_sel, dv, ctx=ctx)
    assert om.shape == (Nn,) and np.all(np.isfinite(om)) and np.all(om >= 0) and np.any(om > 0)
    r = abcutil.particle_ranking_PLS_targets_draws(Xn, theta, Xn[:5], 0.5, 200, S=64, exclude=np.arange(5), max_comp=A, rule=0, ctx=ctx,
                                                   row_weights=om)
    print("generation table: ess of the draws", r["ess"])
    assert np.all(np.isfinite(r["ess"])) and np.all(r["ess"] > 0) and np.all(np.isfinite(r["draws"]))
    a = abcutil.particle_ranking_PLS_targets_adjust(Xn, theta, Xn[:5], 0.5, 200, exclude=np.arange(5), max_comp=A, rule=0, ctx=ctx,
                                                    row_weights=om)
    assert np.all(np.isfinite(a["post_mean"])) and not np.any(a["status"] & 4)
