"""Log and logit parameter transforms of the local-linear adjustment (abc_ctx_set_param_transf, abc_param_transf*): the fit under
a setting is the plain fit on forward(Y) bit for bit and its adjusted rows are that fit's rows carried back; every product under
method 1 sees those rows (the products' own tests run again under a setting, with their own bounds); the path; nothing that does
not regress moves; out-of-domain entries make their own (target, parameter) NaN and nothing else; the adjusted rows stay inside
the support where the plain ones leave it; the transform kernels against the long-double definition; the refusals.

The setting lives in the context the whole suite shares, so every test sets it inside Context.param_transf(...), which restores
what was there before."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_density as TDN
import test_gpu_draws as TDR
import test_gpu_joint as TJ
import test_gpu_summary as TS
from test_gpu_adjust import _fit, _with_nc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def _wl(M, P, N, seed):
    from abcsmc_amd import synthetic
    X, Y = synthetic.Workload(M, P, seed).rows(0, N)
    return np.asarray(X), np.asarray(Y)


def _unit(Y):
    """every column brought into [0.1, 0.9]: inside the domain of every kind of _setting"""
    Y = np.asarray(Y, dtype=np.float64)
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    return np.ascontiguousarray(0.1 + 0.8 * (Y - lo) / (hi - lo))


def _setting(P):
    """kinds mixed per column (logit, none, log, logit, ...) and the logit bounds, each around [0.1, 0.9]"""
    kinds = [("logit", "none", "log")[j % 3] for j in range(P)]
    lo = np.array([0.05 - 0.01 * j for j in range(P)])
    hi = np.array([1.0 + 0.1 * j for j in range(P)])
    return kinds, lo, hi


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _back_rows(ctx, theta):
    """device.param_transf(inverse=True) over adjusted rows (B, K, P) -> the same shape (host)"""
    import torch
    from abcsmc_amd import device
    B, K, P = theta.shape
    h = torch.tensor(np.ascontiguousarray(theta.reshape(B * K, P).T), device=DEV)
    out = device.param_transf(h, inverse=True, ctx=ctx)
    torch.cuda.synchronize()
    return np.ascontiguousarray(out.cpu().numpy().T).reshape(B, K, P)


# ---- 1. the same bits as the plain call on transformed Y ----------------------------------------------------------------------
@pytest.mark.parametrize("N,M,P,K,B", [(800, 5, 4, 1, 4), (2000, 6, 3, 500, 12), (5000, 8, 6, 4097, 3), (1200, 4, 2, 64, 300)])
def test_same_bits_as_plain_call_on_transformed_y(ctx, N, M, P, K, B):
    import torch
    from abcsmc_amd import device
    X, Y = _wl(M, P, N, 7 * N + K)
    Y = _unit(Y)
    F = _fit(ctx, X, Y, min(M, P))
    kinds, lo, hi = _setting(P)
    assert "none" in kinds and "logit" in kinds
    rows = (np.arange(B) * 5) % N
    Td = device.colmajor(X[rows], DEV)
    ybig = torch.full((P, N + 3), float("nan"), dtype=torch.float64, device=DEV)
    ybig[:, 2:N + 2] = F["Yd"]
    Yv = ybig[:, 2:N + 2]                                                # ldy = N + 3
    assert Yv.stride(0) == N + 3
    ctx.param_transf_outside(reset=True)
    with ctx.param_transf(kinds, lo, hi):
        Yt = device.param_transf(Yv, ctx=ctx)
        assert torch.equal(device.param_transf(F["Yd"], ctx=ctx).view(torch.int64), Yt.view(torch.int64))     # ldy plays no part
    assert torch.isfinite(Yt).all() and ctx.param_transf_outside() == 0
    none = [j for j, k in enumerate(kinds) if k == "none"]
    assert torch.equal(Yt[none].view(torch.int64), F["Yd"][none].view(torch.int64))
    for kernel in (0, 1):
        for ex in (None, torch.tensor(rows)):
            with ctx.param_transf(kinds, lo, hi):
                g = _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, Yv, exclude=ex, kernel=kernel, ctx=ctx))
                idx, dist, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], exclude=ex, ctx=ctx)
            p = _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, Yt, exclude=ex, kernel=kernel, ctx=ctx))
            for k in ("coef", "rank", "status", "weight"):
                assert np.array_equal(g[k], p[k], equal_nan=True), (k, kernel, ex is not None)
            assert _same(g["idx"], idx.cpu().numpy()) and _same(g["dist"], dist.cpu().numpy())
            with ctx.param_transf(kinds, lo, hi):
                back = _back_rows(ctx, p["theta"])
            assert np.array_equal(g["theta"], back, equal_nan=True), (kernel, ex is not None)
            assert np.all(np.isfinite(g["theta"])) and np.all(np.isfinite(g["coef"]))
            if K == 1 and kernel == 0:
                assert np.all(g["status"] & 2)                           # the rectangular fallback
            for j, k in enumerate(kinds):
                if k == "log":
                    assert np.all(g["theta"][:, :, j] > 0.0)
                elif k == "logit":
                    assert np.all((g["theta"][:, :, j] >= lo[j]) & (g["theta"][:, :, j] <= hi[j]))
                else:
                    assert _same(g["theta"][:, :, j], p["theta"][:, :, j])


# ---- 2. the products against the adjusted rows: their own tests, under a setting -------------------------------------------
class _Spy:
    """records alpha (coef[:, 0]) of every device.rank_targets_adjust call made while a product's own test runs"""

    def __init__(self, monkeypatch):
        from abcsmc_amd import device
        self.alpha, real = [], device.rank_targets_adjust

        def spy(*a, **kw):
            r = real(*a, **kw)
            self.alpha.append(r["coef"][:, 0].cpu().numpy())
            return r
        monkeypatch.setattr(device, "rank_targets_adjust", spy)

    def check(self, kinds):
        """the fit really ran on the transformed scale: the data lie in [0.1, 0.9], so alpha of a log column is negative"""
        assert self.alpha
        j = kinds.index("log")
        for a in self.alpha:
            assert np.all(a[:, j] < 0.0)


def _unit_wl(mod, monkeypatch):
    real = mod._wl

    def wl(M, P, N, seed):
        X, Y = real(M, P, N, seed)
        return X, _unit(Y)
    monkeypatch.setattr(mod, "_wl", wl)


@pytest.mark.parametrize("kernel", [0, 1])
def test_summary_against_adjusted_rows(ctx, monkeypatch, kernel):
    N, M, P, K, B = 2000, 6, 3, 500, 12
    kinds, lo, hi = _setting(P)
    _unit_wl(TS, monkeypatch)
    spy = _Spy(monkeypatch)
    ctx.param_transf_outside(reset=True)
    with ctx.param_transf(kinds, lo, hi):
        TS.test_loclinear_against_adjusted_rows(ctx, kernel, N, M, P, K, B)
    spy.check(kinds)
    assert ctx.param_transf_outside() == 0


def test_summary_past_the_lds_path(ctx, monkeypatch):
    N, M, P, K, B = 5000, 8, 6, 4097, 3
    kinds, lo, hi = _setting(P)
    _unit_wl(TS, monkeypatch)
    spy = _Spy(monkeypatch)
    with ctx.param_transf(kinds, lo, hi):
        TS.test_loclinear_against_adjusted_rows(ctx, 0, N, M, P, K, B)
    spy.check(kinds)


@pytest.mark.parametrize("kernel", [0, 1])
def test_density_against_adjusted_rows(ctx, monkeypatch, kernel):
    N, M, P, K, B, G = 2000, 6, 3, 500, 12, 512
    kinds, lo, hi = _setting(P)
    _unit_wl(TDN, monkeypatch)
    spy = _Spy(monkeypatch)
    with ctx.param_transf(kinds, lo, hi):
        TDN.test_loclinear_against_adjusted_rows(ctx, kernel, N, M, P, K, B, G)
    spy.check(kinds)


@pytest.mark.parametrize("kernel", [0, 1])
def test_joint_against_adjusted_rows(ctx, monkeypatch, kernel):
    N, M, P, K, B, G, excl, pairs = 2000, 6, 3, 257, 3, 64, True, None
    kinds, lo, hi = _setting(P)
    _unit_wl(TJ, monkeypatch)
    spy = _Spy(monkeypatch)
    with ctx.param_transf(kinds, lo, hi):
        TJ.test_loclinear_against_adjusted_rows(ctx, kernel, N, M, P, K, B, G, excl, pairs)
    spy.check(kinds)


@pytest.mark.parametrize("P,K,S,B,method,kernel,smooth", [(3, 64, 4096, 17, 1, 0, 0), (5, 257, 4096, 17, 1, 0, 1)])
def test_draws_against_reference(ctx, monkeypatch, P, K, S, B, method, kernel, smooth):
    """plain and smoothed draws: test_gpu_draws.py's case on its own set with the parameters brought into the domain"""
    import torch
    from abcsmc_amd import _lib, device
    assert (P, K, S, B, method, kernel, smooth) in TDR.TARGET_CASES
    F0 = TDR._fit(ctx, P)
    Y = np.asfortranarray(_unit(F0["Y"]))
    F = _fit(ctx, np.ascontiguousarray(F0["X"]), np.ascontiguousarray(Y), F0["A"])
    F2 = dict(F0, Y=Y, Yd=F["Yd"], model=F["model"])
    monkeypatch.setitem(TDR._FITS, P, F2)
    kinds, lo, hi = _setting(P)
    spy = _Spy(monkeypatch)
    with ctx.param_transf(kinds, lo, hi):
        TDR.test_targets_against_reference(ctx, P, K, S, B, method, kernel, smooth)
    spy.check(kinds)


@pytest.mark.parametrize("kernel", [0, 1])
def test_path_summary_against_adjusted_rows(ctx, kernel):
    """tolerance t of the path summary against _summary_ref on theta and weight of the adjust call with K = K_t under the same
    setting (test_gpu_summary.py's checks: bit for bit with equal weights, its bounds otherwise)"""
    import torch
    from abcsmc_amd import device
    N, M, P, B, Ks = 2000, 6, 3, 6, (3, 64, 257)
    X, Y = _wl(M, P, N, 77)
    Y = _unit(Y)
    F = _fit(ctx, X, Y, min(M, P))
    kinds, lo, hi = _setting(P)
    rows = np.arange(B) * 5
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    truth = Y[rows].copy()
    with ctx.param_transf(kinds, lo, hi):
        g = _np(device.rank_targets_path_summary(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], probs=TS.PROBS,
                                                 truth=torch.tensor(truth), method=1, kernel=kernel, exclude=ex, ctx=ctx))
        for t, K in enumerate(Ks):
            a = _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
            assert np.all(a["coef"][:, 0, kinds.index("log")] < 0.0)
            for b in range(B):
                rect = kernel == 1 or bool(a["status"][b] & 2)
                (TS._check_exact if rect else TS._check_bounds)(a["theta"][b:b + 1], a["weight"][b:b + 1], g["quant"][b:b + 1, t],
                                                               g["cdf"][b:b + 1, t], truth[b:b + 1])


# ---- 3. the path ------------------------------------------------------------------------------------------------------------------
def test_path_is_the_adjustment_at_every_tolerance(ctx):
    import torch
    from abcsmc_amd import device
    N, M, P, B, Ks = 2000, 6, 3, 7, (3, 64, 257)
    X, Y = _wl(M, P, N, 78)
    Y = _unit(Y)
    F = _fit(ctx, X, Y, min(M, P))
    kinds, lo, hi = _setting(P)
    rows = np.arange(B) * 11
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    for kernel in (0, 1):
        plain = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
        with ctx.param_transf(kinds, lo, hi):
            g = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
            for t, K in enumerate(Ks):
                a = _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], exclude=ex, kernel=kernel,
                                                   theta=False, weight=False, ctx=ctx))
                assert _same(g["idx"][:, :K], a["idx"]) and _same(g["dist"][:, :K], a["dist"])
                assert _same(g["coef"][:, t], a["coef"]), (kernel, K)
                assert np.array_equal(g["rank"][:, t], a["rank"]) and np.array_equal(g["status"][:, t], a["status"])
        for k in ("post_mean", "h", "idx", "dist"):
            assert _same(g[k], plain[k]), k
        assert not _same(g["coef"], plain["coef"])


# ---- 4. nothing else moves ------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(ctx):
    import torch
    from abcsmc_amd import abcutil, device
    N, M, P, K, B = 3000, 6, 3, 500, 5
    X, Y = _wl(M, P, N, 79)
    Y = _unit(Y)
    F = _fit(ctx, X, Y, 3)
    kinds, lo, hi = _setting(P)
    rows = np.arange(B) * 7
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    args = (F["Xd"], F["model"], F["A"], Td)
    rng = np.random.default_rng(3)
    V = torch.tensor(rng.normal(size=(P, 700)), device=DEV)
    w = torch.tensor(rng.uniform(0, 1, 700), device=DEV)

    def calls():
        r = {}
        idx, dist, pm = device.rank_targets(*args, K, Y=F["Yd"], exclude=ex, post_mean=True, ctx=ctx)
        r["rank"] = dict(idx=idx, dist=dist, pm=pm)
        r["summary"] = device.rank_targets_summary(*args, K, F["Yd"], truth=torch.tensor(Y[rows]), exclude=ex, dist=True, ctx=ctx)
        r["density"] = device.rank_targets_density(*args, K, F["Yd"], G=65, exclude=ex, ctx=ctx)
        r["joint"] = device.rank_targets_joint(*args, K, F["Yd"], G=16, exclude=ex, ctx=ctx)
        r["draws"] = device.rank_targets_draws(*args, K, F["Yd"], 257, smooth=True, seed=5, exclude=ex, ctx=ctx)
        r["path_summary"] = device.rank_targets_path_summary(*args, (3, 64, K), F["Yd"], exclude=ex, coef=False, fit=False, ctx=ctx)
        r["w_summary"] = device.weighted_summary(V, w, ctx=ctx)
        r["w_density"] = device.weighted_density(V, w, G=65, ctx=ctx)
        r["w_joint"] = device.weighted_joint(V, w, G=16, ctx=ctx)
        r["w_draws"] = device.weighted_draws(V, w, S=257, smooth=True, seed=5, ctx=ctx)
        return {k: _np(v) for k, v in r.items()}

    adjust = lambda T=Td, e=ex: _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], T, K, F["Yd"], exclude=e, ctx=ctx))
    before, a_before = calls(), adjust()
    with ctx.param_transf(kinds, lo, hi):
        during, a_during = calls(), adjust()
        # alone and in a batch, and through the host entry (the same fit: rule 0, A = 3)
        for b in (0, B - 1):
            one = adjust(device.colmajor(X[rows[b:b + 1]], DEV), ex[b:b + 1])
            for k in ("idx", "dist", "theta", "weight", "coef", "rank", "status"):
                assert _same(one[k][0], a_during[k][b]), (k, b)
    host = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[rows], 0.5, K, exclude=rows, max_comp=3, rule=0, ctx=ctx,
                                                       transf=kinds, bounds=np.stack([lo, hi], axis=1))
    a_after = adjust()
    for name in before:
        for k in before[name]:
            if isinstance(before[name][k], np.ndarray):
                assert _same(before[name][k], during[name][k]), (name, k)
    for k in a_before:
        assert _same(a_before[k], a_after[k]), k
    assert not _same(a_before["theta"], a_during["theta"]) and _same(a_before["weight"], a_during["weight"])
    assert host["ncomp"] == F["ncomp"]
    for k in ("theta", "weight", "coef", "rank", "status"):
        assert _same(host[k], a_during[k]), k
    assert _same(host["idx"].astype(np.int64), a_during["idx"])
    assert np.array_equal(host["post_mean"], abcutil.untransform_params(a_during["coef"][:, 0], kinds, np.stack([lo, hi], axis=1)))
    assert getattr(ctx, "_transf", None) is None                         # the wrapper restored the context


# ---- 5. the domain ---------------------------------------------------------------------------------------------------------------
def test_out_of_domain_entries(ctx):
    import torch
    from abcsmc_amd import device
    N, M, P, K, B = 1500, 5, 3, 200, 6
    X, Y = _wl(M, P, N, 80)
    Y = _unit(Y)
    kinds, lo, hi = ["log", "none", "logit"], np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.25])
    F = _fit(ctx, X, Y, 3)
    model = _with_nc(F, 2)
    rows = np.arange(B) * 9
    Td = device.colmajor(X[rows], DEV)
    probs = (0.025, 0.5, 0.975)

    def run(Yd):
        with ctx.param_transf(kinds, lo, hi):
            return _np(device.rank_targets_summary(F["Xd"], model, F["A"], Td, K, Yd, probs=probs, method=1, dist=True,
                                                   adjust=("theta", "weight", "coef", "rank", "status"), ctx=ctx))
    ctx.param_transf_outside(reset=True)
    clean = run(F["Yd"])
    assert ctx.param_transf_outside() == 0 and np.all(clean["rank"] == 2)
    i = int(clean["idx"][0, 5])
    kept = set(clean["idx"].reshape(-1).tolist())
    away = [r for r in range(N) if r not in kept][:4]
    assert len(away) == 4
    Yb = np.array(Y)
    Yb[i, 0], Yb[i, 2] = -1.0, hi[2]                                     # a retained row: -1 under log, hi under logit
    Yb[away[0], 0], Yb[away[1], 0], Yb[away[2], 2], Yb[away[3], 2] = 0.0, np.inf, 0.0, np.nan     # rows nobody retains
    Yb[away[0], 1] = -5.0                                                # a NONE column has no domain
    bad = run(device.colmajor(Yb, DEV))
    assert ctx.param_transf_outside() == 6
    assert ctx.param_transf_outside(reset=True) == 6 and ctx.param_transf_outside() == 0
    hit = np.array([i in clean["idx"][b] for b in range(B)])
    assert hit[0] and not hit.all()
    for k in ("idx", "dist", "weight", "rank", "status"):
        assert _same(bad[k], clean[k]), k
    for b in range(B):
        for j in range(P):
            nan = hit[b] and j in (0, 2)
            if nan:
                assert np.isnan(bad["coef"][b, :3, j]).all() and np.isnan(bad["theta"][b, :, j]).all()
                assert np.isnan(bad["quant"][b, :, j]).all()
            else:
                assert _same(bad["coef"][b, :, j], clean["coef"][b, :, j]) and _same(bad["theta"][b, :, j], clean["theta"][b, :, j])
                assert _same(bad["quant"][b, :, j], clean["quant"][b, :, j])


# ---- 6. the support ------------------------------------------------------------------------------------------------------------
def test_adjusted_rows_stay_inside_the_support(ctx):
    """parameters made as in tests/test_transf_cpu.py (the back-transform of linear in the metrics + noise): the plain adjustment
    leaves the support, the transformed one does not, and neither do its 2.5 % and 97.5 % quantiles"""
    import torch
    from abcsmc_amd import device
    N, M, P, K, B = 3000, 5, 4, 1000, 8
    rng = np.random.default_rng(21)
    X = rng.standard_normal((N, M))
    eta = X @ rng.normal(0.0, 0.8, (M, P)) + 0.3 * rng.standard_normal((N, P))
    kinds = ["log", "logit", "log", "logit"]
    lo, hi = np.array([0.0, -1.0, 0.0, -1.0]), np.array([0.0, 3.0, 0.0, 3.0])
    Y = np.where(np.array(kinds) == "log", np.exp(eta), -1.0 + 4.0 / (1.0 + np.exp(-1.5 * eta)))
    inf = np.where(np.array(kinds) == "log", np.inf, hi)
    assert np.all((Y > lo) & (Y < inf))
    F = _fit(ctx, X, np.ascontiguousarray(Y), 3)
    Td = device.colmajor(X[np.arange(B) * 13], DEV)
    plain = _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], ctx=ctx))
    pos = plain["weight"] > 0
    out = (plain["theta"] <= lo) | (plain["theta"] >= inf)
    assert (out & pos[:, :, None]).sum() >= 1, "the plain adjustment stays inside the support: the case shows nothing"
    with ctx.param_transf(kinds, lo, hi):
        g = _np(device.rank_targets_summary(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], probs=(0.025, 0.975), method=1,
                                            adjust=("theta", "weight"), ctx=ctx))
    assert np.all(np.isfinite(g["theta"]))
    th = g["theta"][g["weight"] > 0]
    assert not ((th <= lo) | (th >= inf)).any()
    q = g["quant"]
    assert np.all((q > lo) & (q < inf))


# ---- 7. accuracy of the transform kernels -------------------------------------------------------------------------------------
def _values(n, kind, lo, hi, inverse, rng):
    """n inputs: the hard ones first (near the bounds, near 1 under log, |t| up to 700), then random ones"""
    if inverse:
        hard = [0.0, -0.0, 700.0, -700.0, 1e-300, -1e-17, 36.7, -36.7, 0.5, 650.0]
        v = np.concatenate([hard, rng.uniform(-700, 700, n)])
    elif kind == "log":
        one = 1.0 + np.arange(-4, 5) * np.spacing(1.0)
        v = np.concatenate([one, [1.0 + 1e-8, 1.0 - 1e-8, 1e-300, 1e300], np.exp(rng.uniform(-700, 700, n))])
    elif kind == "logit":
        k = np.arange(1, 5)
        v = np.concatenate([lo + k * np.spacing(abs(lo)), hi - k * np.spacing(abs(hi)), [0.5 * (lo + hi)], rng.uniform(lo, hi, n)])
        v = v[(v > lo) & (v < hi)]
    else:
        v = np.concatenate([[-0.0, 0.0, np.inf, -np.inf, np.nan], rng.normal(0, 100, n)])
    return np.resize(v, n) if n >= 1 else v


@pytest.mark.parametrize("n", [1, 63, 1000])
def test_transform_kernels_against_long_double(ctx, n):
    """device.param_transf, both directions, against the definition in np.longdouble on the same fp64 inputs.  The model, fixed
    before any run (u(x) = the spacing of fp64 at |x|, eps = 2^-53):
      HIP's published table of double-precision math functions gives log and exp a maximum error of 1 ulp each (the figure
      used here is that published one, not one read from an installed copy of the documentation); the long-double reference
      rounded to fp64 costs another half ulp, and its own long-double roundings (3 x 2^-64 relative on the logit's ratio) ride
      along.
      forward log    |t - log y|              <= 1.5 u(t)
      forward logit  the two subtractions and the division put a relative 3 eps (1 + 2^-50) on the ratio, which enters t
                     absolutely; then the logarithm:  <= 3 eps (1 + 2^-50) + 3 x 2^-64 + 1.5 u(t)
      back log       |y - exp t|              <= 1.5 u(y)
      back logit     e = exp(-t): relative 2 eps; d = 1 + e: the error of e weighs e / d <= 1, plus eps; s = 1 / d: plus eps; hi - lo:
                     plus eps; so (hi - lo) s carries a relative 5 eps (1 + 2^-40), then the fma's rounding and the reference's:
                     <= 5 eps (1 + 2^-40) (hi - lo) s + 1.0 u(y).  The clamp only moves a value towards the exact one, which
                     lies in [lo, hi].
      none           bit for bit."""
    import torch
    from abcsmc_amd import abcutil, device
    kinds, lo, hi = ["log", "logit", "none", "logit"], np.array([0.0, -1.0, 0.0, 0.25]), np.array([0.0, 3.0, 0.0, 0.75])
    bounds = np.stack([lo, hi], axis=1)
    P, eps = 4, 2.0 ** -53
    rng = np.random.default_rng(n)
    for inverse in (False, True):
        V = np.stack([_values(n, kinds[j], lo[j], hi[j], inverse, rng) for j in range(P)], axis=1)      # (n, P)
        big = torch.full((P, n + 3), float("nan"), dtype=torch.float64, device=DEV)
        big[:, :n] = torch.tensor(np.ascontiguousarray(V.T))
        with ctx.param_transf(kinds, lo, hi):
            out = device.param_transf(big[:, :n], inverse=inverse, ctx=ctx)                             # ldv = n + 3
        torch.cuda.synchronize()
        got = out.cpu().numpy().T
        ref = (abcutil.untransform_params if inverse else abcutil.transform_params)(V.astype(LD), kinds, bounds)
        assert _same(got[:, 2], V[:, 2])
        u = lambda x: np.spacing(np.abs(x.astype(np.float64)))
        for j in (0, 1, 3):
            r = ref[:, j]
            assert np.all(np.isfinite(r.astype(np.float64)))
            err = np.abs(got[:, j].astype(LD) - r)
            if not inverse and kinds[j] == "log":
                tol = 1.5 * u(r)
            elif not inverse:
                tol = 3 * eps * (1 + 2.0 ** -50) + 3 * 2.0 ** -64 + 1.5 * u(r)
            elif kinds[j] == "log":
                tol = 1.5 * u(r)
            else:
                s = 1 / (1 + np.exp(-V[:, j].astype(LD)))
                tol = 5 * eps * (1 + 2.0 ** -40) * (hi[j] - lo[j]) * s + 1.0 * u(r)
                assert np.all((got[:, j] >= lo[j]) & (got[:, j] <= hi[j]))
            worst = float((err / tol.astype(LD)).max())
            print("n=%d %s %s: worst error / bound %.3f" % (n, "back" if inverse else "forward", kinds[j], worst))
            assert np.all(err <= tol), (inverse, kinds[j], worst)
    # with nothing set it copies, bit for bit
    out = device.param_transf(big[:, :n], ctx=ctx)
    assert torch.equal(out.view(torch.int64), big[:, :n].contiguous().view(torch.int64))
    # the infinities of the back direction
    with ctx.param_transf(kinds, lo, hi):
        t = torch.tensor([[np.inf, -np.inf, np.nan]] * P, dtype=torch.float64, device=DEV)
        y = device.param_transf(t, inverse=True, ctx=ctx).cpu().numpy()
    assert y[0, 0] == np.inf and y[0, 1] == 0.0 and np.isnan(y[:, 2]).all()
    assert np.array_equal(y[1, :2], [3.0, -1.0]) and np.array_equal(y[3, :2], [0.75, 0.25])


def test_host_entry_and_in_place(ctx):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    kinds, lo, hi = _setting(3)
    rng = np.random.default_rng(5)
    V = np.asfortranarray(rng.uniform(0.1, 0.9, (257, 3)))
    out = np.empty_like(V)
    with ctx.param_transf(kinds, lo, hi):
        ctx.check(L.abc_param_transf(ctx.handle, V.ctypes.data, 257, 3, 0, out.ctypes.data))
        d = device.colmajor(V, DEV)
        fwd = device.param_transf(d, ctx=ctx)
        ctx.check(L.abc_param_transf_dev(ctx.handle, d.data_ptr(), 257, 257, 3, 0, d.data_ptr(), 257))      # in place
        torch.cuda.synchronize()
    assert _same(out.T, fwd.cpu().numpy()) and torch.equal(d, fwd)


# ---- 8. the refusals ------------------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()

    def refused(rc):
        assert rc == INVALID, rc
        assert L.abc_last_error(ctx.handle)

    def setting(P, kind, lo, hi):
        k = np.asarray(kind, dtype=np.int32)
        l = None if lo is None else np.asarray(lo, dtype=np.float64)
        h = None if hi is None else np.asarray(hi, dtype=np.float64)
        tf = _lib.ParamTransf(P, k.ctypes.data, None if l is None else l.ctypes.data, None if h is None else h.ctypes.data)
        return L.abc_ctx_set_param_transf(ctx.handle, C.byref(tf))

    refused(setting(1025, [1] * 1025, None, None))
    refused(setting(2, [0, 3], None, None))
    refused(setting(2, [-1, 0], None, None))
    refused(setting(2, [2, 0], None, None))                                  # logit without bounds
    refused(setting(2, [2, 0], [0.0, 0.0], None))
    refused(setting(2, [2, 0], [0.0, 0.0], [np.inf, 1.0]))
    refused(setting(2, [2, 0], [np.nan, 0.0], [1.0, 1.0]))
    refused(setting(2, [2, 0], [1.0, 0.0], [1.0, 1.0]))                      # not lo < hi
    refused(setting(2, [0, 2], [0.0, 2.0], [1.0, 1.0]))
    refused(L.abc_ctx_set_param_transf(ctx.handle, C.byref(_lib.ParamTransf(2, None, None, None))))
    assert setting(2, [0, 0], None, None) == 0 and setting(2, [1, 0], None, None) == 0      # bounds of non-logit entries are not read
    assert L.abc_ctx_set_param_transf(ctx.handle, None) == 0

    N, M, P, K, B = 500, 5, 3, 10, 4
    X, Y = _wl(M, P, N, 81)
    Y = _unit(Y)
    F = _fit(ctx, X, Y, 3)
    Td = device.colmajor(X[:B], DEV)
    a = (F["Xd"], F["model"], F["A"], Td)
    with ctx.param_transf(["log", "none"]):                                  # a setting for two parameters, calls with three
        for call in (lambda: device.rank_targets_adjust(*a, K, F["Yd"], ctx=ctx),
                     lambda: device.rank_targets_path(*a, (3, K), F["Yd"], ctx=ctx),
                     lambda: device.rank_targets_path_summary(*a, (3, K), F["Yd"], method=1, ctx=ctx),
                     lambda: device.rank_targets_summary(*a, K, F["Yd"], method=1, ctx=ctx),
                     lambda: device.rank_targets_density(*a, K, F["Yd"], G=16, method=1, ctx=ctx),
                     lambda: device.rank_targets_joint(*a, K, F["Yd"], G=16, method=1, ctx=ctx),
                     lambda: device.rank_targets_draws(*a, K, F["Yd"], 8, method=1, ctx=ctx),
                     lambda: device.param_transf(F["Yd"], ctx=ctx)):
            with pytest.raises(_lib.AbcError) as e:
                call()
            assert e.value.code == INVALID and "parameter transforms" in str(e.value)
        # nothing was queued: the outputs of a refused call are untouched
        idx = torch.full((B, K), -7, dtype=torch.int64, device=DEV)
        out = _lib.AdjustOut(None, None, None, None, None)
        refused(L.abc_rank_targets_adjust_dev(ctx.handle, F["Xd"].data_ptr(), N, F["Yd"].data_ptr(), N, N, M, P,
                                              F["model"].data_ptr(), F["A"], Td.data_ptr(), B, B, None, K, 0, idx.data_ptr(), None,
                                              C.byref(out)))
        torch.cuda.synchronize()
        assert torch.all(idx == -7)
        # the host forms
        from abcsmc_amd import abcutil
        with pytest.raises(_lib.AbcError):
            abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:B], 0.5, K, max_comp=3, rule=0, ctx=ctx)
        with pytest.raises(_lib.AbcError):
            abcutil.particle_ranking_PLS_targets_summary(X, Y, X[:B], 0.5, K, method="loclinear", max_comp=3, rule=0, ctx=ctx)
        # calls that do not regress ignore the setting
        device.rank_targets(*a, K, Y=F["Yd"], ctx=ctx)
        device.rank_targets_summary(*a, K, F["Yd"], ctx=ctx)
        abcutil.particle_ranking_PLS_targets(X, Y, X[:B], 0.5, K, max_comp=3, rule=0, ctx=ctx)
    # the other refusals of abc_param_transf_dev
    d = F["Yd"]
    refused(L.abc_param_transf_dev(ctx.handle, None, N, N, P, 0, d.data_ptr(), N))
    refused(L.abc_param_transf_dev(ctx.handle, d.data_ptr(), N, N, P, 0, None, N))
    refused(L.abc_param_transf_dev(ctx.handle, d.data_ptr(), N - 1, N, P, 0, d.data_ptr(), N))
    refused(L.abc_param_transf_dev(ctx.handle, d.data_ptr(), N, N, P, 0, d.data_ptr(), N - 1))
    # the context stays usable and holds no setting
    g = _np(device.rank_targets_adjust(*a, K, F["Yd"], ctx=ctx))
    assert np.all(np.isfinite(g["theta"])) and getattr(ctx, "_transf", None) is None
