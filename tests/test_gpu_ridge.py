"""Ridge adjustment with the penalty chosen by leave-one-out PRESS (abc_ctx_set_adjust_ridge, abc_adjust_last_ridge,
abc_adjust_ridge_unscored): coef, theta, the picks and PRESS against the NumPy reference of the header's definition
(_ridge_ref); a slot's bits alone, in a batch, through the host entry, through strided views, through both gather paths and
on a tolerance path; lambda = (0,) is the plain call; nothing but coef and theta moves; every product under method 1 sees the
ridge fit (the products' own tests run again under the setting, with their own bounds); the composition with transforms and
the variance correction; the refusals; and the choice lowers the prediction error where rows are few.

The setting lives in the context the whole suite shares, so every test sets it inside Context.adjust_ridge(...), which
restores what was there before."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _hcorr_ref as H
import _loclinear_ref as R
import _ridge_ref as G
from test_gpu_hcorr import _fit, _np, _same, hetero_data

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1
# the penalties are spread widely enough that, at K = 4097 too, two neighbours' PRESS differ by more than the 1e-6 below which a
# pick is not compared (PRESS changes by about lambda nc / K, relatively, between neighbours)
L5 = (0.0, 1e-2, 1e-1, 1.0, 10.0)                                        # L = 5 including 0
L8 = (1e-2, 3e-2, 1e-1, 0.3, 1.0, 3.0, 10.0, 30.0)                       # L = 8 without 0


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def _adjust(ctx, F, model, T, K, lam=L5, exclude=None, kernel=0, Y=None, X=None, hcorr=False, **kw):
    """device.rank_targets_adjust under the setting (lam None: off); returns the host arrays with pick and press added"""
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(T, DEV) if isinstance(T, np.ndarray) else T
    ex = torch.tensor(np.asarray(exclude)) if exclude is not None else None
    with ctx.adjust_ridge(lam), ctx.adjust_hcorr(hcorr):
        g = _np(device.rank_targets_adjust(F["Xd"] if X is None else X, model, F["A"], Td, K, F["Yd"] if Y is None else Y,
                                           exclude=ex, kernel=kernel, ctx=ctx, **kw))
        if lam is not None:
            g["pick"], g["press"] = ctx.last_ridge()
        if hcorr:
            g["hcoef"] = ctx.last_hcorr()
    return g


def _check_ref(F, T, g, b, nc, kernel, lam, tag, Y=None, hcorr=False):
    """coef, theta and the finite PRESS within test_gpu_hcorr.py's bound: 1e-9 of the parameter's range (PRESS: of its own value)
    plus 100x what a relative 1e-15 perturbation of the scores changes in the reference, that widening term below 1e-8; pick
    where the reference's gap between the two smallest PRESS exceeds 1e-6 (the other parameters are counted and left out).
    Returns (pairs left out, the reference)."""
    X, Y = F["X"], F["Y"] if Y is None else Y
    idx = g["idx"][b].astype(np.int64)
    S = R.scores(X[idx], F["mean"], F["sd"], F["R"], nc)
    o = R.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
    Sp = S * (1.0 + 1e-15 * np.random.default_rng(b).standard_normal(S.shape))

    def fit(Sx):
        if not hcorr:
            return G.ridge(g["dist"][b], Sx, o, Y[idx], lam, kernel=kernel, A=F["A"])
        real = R.loclinear                                   # the composed definition: the second fit models the ridge fit's residuals
        R.loclinear = lambda d, S_, o_, th, kernel=0, A=None: G.ridge(d, S_, o_, th, lam, kernel=kernel, A=A)
        try:
            return H.hcorr(g["dist"][b], Sx, o, Y[idx], kernel=kernel, A=F["A"])
        finally:
            R.loclinear = real
    ref, pert = fit(S), fit(Sp)
    span = Y.max(axis=0) - Y.min(axis=0)
    assert g["rank"][b] == ref["rank"] == pert["rank"] and g["status"][b] == ref["status"], (tag, b)
    assert np.array_equal(g["weight"][b], ref["weight"]), (tag, b)
    sure = (ref["gap"] > 1e-6) & (ref["pick"] == pert["pick"])
    print("%s b=%d smallest gap %.3g, pairs left out %d" % (tag, b, ref["gap"].min(), int((~sure).sum())))
    assert np.array_equal(g["pick"][b][sure], ref["pick"][sure]), (tag, b, g["pick"][b], ref["pick"], ref["gap"])
    ok = sure & (g["pick"][b] == ref["pick"])
    fin = np.isfinite(ref["press"])
    assert np.array_equal(np.isfinite(g["press"][b]), fin) and np.array_equal(np.isfinite(pert["press"]), fin), (tag, b)
    assert np.all(g["press"][b][~fin] == np.inf)
    sens = np.abs(pert["press"][fin] - ref["press"][fin])
    err = np.abs(g["press"][b][fin] - ref["press"][fin])
    if fin.any():
        print("%s b=%d press: err/value %.3g, widening/value %.3g" % (tag, b, (err / ref["press"][fin]).max(),
                                                                       (100.0 * sens / ref["press"][fin]).max()))
    assert np.all(100.0 * sens < 1e-8 * ref["press"][fin]), (tag, b, "press", "the case breaks the condition")
    assert np.all(err <= 1e-9 * ref["press"][fin] + 100.0 * sens), (tag, b, "press", (err / ref["press"][fin]).max())
    for key in ("coef", "theta") + (("hcoef",) if hcorr else ()):
        sens = np.abs(pert[key] - ref[key]).max(axis=0)[ok]
        err = np.abs(g[key][b] - ref[key]).max(axis=0)[ok]
        if ok.any():
            print("%s b=%d %s: err/range %.3g, widening/range %.3g" % (tag, b, key, (err / span[ok]).max(),
                                                                        (100.0 * sens / span[ok]).max()))
        assert np.all(100.0 * sens < 1e-8 * span[ok]), (tag, b, key, "the case breaks the condition: other data, not a wider bound")
        assert np.all(err <= 1e-9 * span[ok] + 100.0 * sens), (tag, b, key, (err / span[ok]).max())
    assert np.all(g["coef"][b][1 + nc:] == 0.0)
    return int((~sure).sum()), ref


# the issue's shapes (N, M, P, K, B, comps); the last one (K = nc + 1) has its own test below
CASES = [(800, 5, 4, 16, 4, 0), (2000, 6, 3, 500, 12, 0), (5000, 8, 6, 4097, 3, 0), (1500, 16, 80, 300, 3, 12),
         (1500, 56, 80, 300, 2, 52)]


@pytest.mark.parametrize("N,M,P,K,B,comps", CASES)
def test_against_reference(ctx, N, M, P, K, B, comps):
    from test_gpu_adjust import _with_nc
    X, Y = hetero_data(N, M, P, 3 * N + K)
    A = comps if comps else min(M, P)
    F = _fit(ctx, X, Y, A)
    nc = comps if comps else F["ncomp"]
    model = _with_nc(F, nc)
    rows = (np.arange(B) * 3) % N
    T = np.ascontiguousarray(X[rows])
    left, pairs = 0, 0
    for kernel in (0, 1):
        off = _adjust(ctx, F, model, T, K, None, exclude=rows, kernel=kernel)
        for lam in (L5, L8):
            g = _adjust(ctx, F, model, T, K, lam, exclude=rows, kernel=kernel)
            assert g["pick"].shape == (B, P) and g["press"].shape == (B, len(lam), P)
            for k in ("idx", "dist", "weight", "rank", "status"):       # the fixed outputs
                assert _same(g[k], off[k]), k
            for b in sorted({0, B - 1}):
                n, _ = _check_ref(F, T, g, b, nc, kernel, lam, (N, M, P, K, B, kernel, len(lam)))
                left, pairs = left + n, pairs + P
    assert 100 * left <= pairs, (left, pairs)                            # at most 1 % of the pairs left out of the pick check


def test_k_is_nc_plus_one(ctx):
    """(600, 8, 3, 9, 5, 8): nine rows for nine coefficients, the unpenalised fit interpolates: under lambda = (0,) every PRESS is
    +inf, the pick is L - 1 and the counter moves by B P.  A positive penalty keeps every leverage below 1 by the definition
    (rules 6 to 8), so in L5 only penalty 0 is +inf and in L8 none is; those hold against the reference like any other case."""
    from test_gpu_adjust import _with_nc
    N, M, P, K, B, nc = 600, 8, 3, 9, 5, 8
    X, Y = hetero_data(N, M, P, 3 * N + K)
    F = _fit(ctx, X, Y, nc)
    model = _with_nc(F, nc)
    rows = (np.arange(B) * 3) % N
    T = np.ascontiguousarray(X[rows])
    for kernel in (0, 1):
        ctx.adjust_ridge_unscored(reset=True)
        g = _adjust(ctx, F, model, T, K, (0.0,), exclude=rows, kernel=kernel)
        off = _adjust(ctx, F, model, T, K, None, exclude=rows, kernel=kernel)
        assert np.all(g["press"] == np.inf) and np.all(g["pick"] == 0) and ctx.adjust_ridge_unscored() == B * P
        assert _same(g["coef"], off["coef"]) and _same(g["theta"], off["theta"])
        g = _adjust(ctx, F, model, T, K, L5, exclude=rows, kernel=kernel)
        assert np.all(g["press"][:, 0] == np.inf) and np.all(np.isfinite(g["press"][:, 1:])) and np.all(g["pick"] > 0)
        assert ctx.adjust_ridge_unscored(reset=True) == B * P and ctx.adjust_ridge_unscored() == 0
        for lam in (L5, L8):
            g = _adjust(ctx, F, model, T, K, lam, exclude=rows, kernel=kernel)
            for b in (0, B - 1):
                _check_ref(F, T, g, b, nc, kernel, lam, ("K = nc + 1", kernel, len(lam)))


# ---- the same bits ----------------------------------------------------------------------------------------------------------
def test_alone_in_a_batch_and_through_the_host_entry(ctx):
    import torch
    from abcsmc_amd import abcutil, device
    N, M, P, K, B = 3000, 6, 3, 200, 300
    X, Y = hetero_data(N, M, P, 5)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 7
    T = np.ascontiguousarray(X[rows])
    g = _adjust(ctx, F, F["model"], T, K, exclude=rows)
    host = abcutil.particle_ranking_PLS_targets_adjust(X, Y, T, 0.5, K, exclude=rows, max_comp=3, rule=0, ctx=ctx, ridge=L5)
    assert host["ncomp"] == F["ncomp"] and ctx._ridge == ()              # the wrapper restored the context
    for k in ("theta", "weight", "coef", "rank", "status"):
        assert _same(host[k], g[k]), k
    assert _same(host["ridge_pick"], g["pick"]) and _same(host["ridge_press"], g["press"])
    assert host["ridge_lambda"].tolist() == list(L5) and len(set(g["pick"].ravel().tolist())) > 1
    for b in (0, 5, 123, 299):
        one = _adjust(ctx, F, F["model"], T[b:b + 1], K, exclude=rows[b:b + 1])
        for k in ("idx", "theta", "weight", "coef", "pick", "press"):
            assert _same(one[k][0], g[k][b]), (k, b)
    xbig = torch.full((M, N + 5), float("nan"), dtype=torch.float64, device=DEV)
    ybig = torch.full((P, N + 3), float("nan"), dtype=torch.float64, device=DEV)
    tbig = torch.full((M, B + 2), float("nan"), dtype=torch.float64, device=DEV)
    xbig[:, 1:N + 1], ybig[:, 2:N + 2], tbig[:, 1:B + 1] = F["Xd"], F["Yd"], device.colmajor(T, DEV)
    v = _adjust(ctx, F, F["model"], tbig[:, 1:B + 1], K, exclude=rows, X=xbig[:, 1:N + 1], Y=ybig[:, 2:N + 2])
    for k in ("idx", "theta", "weight", "coef", "pick", "press"):
        assert _same(v[k], g[k]), k


def test_table_and_direct_gather_agree(tmp_path):
    """ABC_ADJ_GATHER=table / direct (ABC_DIAG=1), each in a fresh process: the same bits through both gather paths"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for path in ("table", "direct"):
        out = str(tmp_path / (path + ".npz"))
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "_ridge_worker.py"), out], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, ABC_DIAG="1", ABC_ADJ_GATHER=path), cwd=root)
        assert p.returncode == 0, p.stderr[-3000:]
        res[path] = dict(np.load(out))
    assert len(res["table"]) == 12
    for k in res["table"]:
        assert _same(res["table"][k], res["direct"][k]), k
    assert np.all(np.isfinite(res["table"]["e_ridge_press"]))


def test_lambda_zero_and_the_fixed_outputs(ctx):
    """lambda = (0,): coef, theta, rank and status are the bits of the call with the setting off; with any list idx, dist,
    weight, rank and status are; and the call with the setting off again has today's bits"""
    N, M, P, K, B = 3000, 6, 3, 500, 5
    X, Y = hetero_data(N, M, P, 79)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 7
    T = np.ascontiguousarray(X[rows])
    for kernel in (0, 1):
        off = _adjust(ctx, F, F["model"], T, K, None, exclude=rows, kernel=kernel)
        zero = _adjust(ctx, F, F["model"], T, K, (0.0,), exclude=rows, kernel=kernel)
        for k in off:
            assert _same(off[k], zero[k]), k
        assert np.all(zero["pick"] == 0) and np.all(np.isfinite(zero["press"])) and zero["press"].shape == (B, 1, P)
        big = _adjust(ctx, F, F["model"], T, K, (5.0, 50.0), exclude=rows, kernel=kernel)
        for k in ("idx", "dist", "weight", "rank", "status"):
            assert _same(off[k], big[k]), k
        assert not _same(off["coef"], big["coef"]) and not _same(off["theta"], big["theta"])
        again = _adjust(ctx, F, F["model"], T, K, None, exclude=rows, kernel=kernel)
        for k in off:
            assert _same(off[k], again[k]), k


def test_method_zero_and_the_generic_entries_do_not_move(ctx):
    import torch
    from abcsmc_amd import device
    N, M, P, K, B = 3000, 6, 3, 500, 5
    X, Y = hetero_data(N, M, P, 79)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 7
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    args = (F["Xd"], F["model"], F["A"], Td)

    def calls():
        r = {}
        idx, dist, pm = device.rank_targets(*args, K, Y=F["Yd"], exclude=ex, post_mean=True, ctx=ctx)
        r["rank"] = dict(idx=idx, dist=dist, pm=pm)
        r["summary"] = device.rank_targets_summary(*args, K, F["Yd"], truth=torch.tensor(Y[rows]), exclude=ex, dist=True, ctx=ctx)
        r["density"] = device.rank_targets_density(*args, K, F["Yd"], G=65, exclude=ex, ctx=ctx)
        r["joint"] = device.rank_targets_joint(*args, K, F["Yd"], G=16, exclude=ex, ctx=ctx)
        r["draws"] = device.rank_targets_draws(*args, K, F["Yd"], 257, smooth=True, seed=5, exclude=ex, ctx=ctx)
        r["path_summary"] = device.rank_targets_path_summary(*args, (3, 64, K), F["Yd"], exclude=ex, coef=False, fit=False, ctx=ctx)
        return {k: _np(v) for k, v in r.items()}

    before = calls()
    with ctx.adjust_ridge(L5):
        during = calls()
    for name in before:
        for k in before[name]:
            if isinstance(before[name][k], np.ndarray):
                assert _same(before[name][k], during[name][k]), (name, k)


# ---- the tolerance path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1])
def test_path_slots_are_the_adjustment_at_every_tolerance(ctx, kernel):
    import torch
    from abcsmc_amd import device
    N, M, P, B, Ks = 3000, 6, 3, 5, (64, 257, 1000)
    X, Y = hetero_data(N, M, P, 6)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 11
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    plain = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
    with ctx.adjust_ridge(L5):
        g = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
        pick, press = ctx.last_ridge()
    assert pick.shape == (B * len(Ks), P) and press.shape == (B * len(Ks), len(L5), P)
    pick, press = pick.reshape(B, len(Ks), P), press.reshape(B, len(Ks), len(L5), P)
    for k in ("post_mean", "h", "idx", "dist", "rank", "status"):
        assert _same(plain[k], g[k]), k
    assert not _same(plain["coef"], g["coef"])
    for t, K in enumerate(Ks):
        a = _adjust(ctx, F, F["model"], Td, K, exclude=rows, kernel=kernel)
        assert _same(g["coef"][:, t], a["coef"]), (kernel, K)
        assert _same(pick[:, t], a["pick"]) and _same(press[:, t], a["press"]), (kernel, K)


# ---- the products: their own tests, under the setting ------------------------------------------------------------------------
class _Spy:
    """checks that every device.rank_targets_adjust call made while a product's own test runs was made with the ridge fit"""

    def __init__(self, monkeypatch, ctx):
        from abcsmc_amd import device
        self.n, real = 0, device.rank_targets_adjust

        def spy(*a, **kw):
            r = real(*a, **kw)
            pick, _ = ctx.last_ridge()
            assert pick.shape[0] == r["coef"].shape[0]
            with ctx.adjust_ridge(None):
                off = real(*a, **kw)
            assert not _same(off["theta"].cpu().numpy(), r["theta"].cpu().numpy())
            assert not _same(off["coef"].cpu().numpy(), r["coef"].cpu().numpy())
            self.n += 1
            return r
        monkeypatch.setattr(device, "rank_targets_adjust", spy)


LP = (0.5, 2.0)                                                          # no zero: every fit differs from the plain one


def test_summary_against_ridge_rows(ctx, monkeypatch):
    import test_gpu_summary as TS
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_ridge(LP):
        TS.test_loclinear_against_adjusted_rows(ctx, 0, 2000, 6, 3, 500, 12)
    assert spy.n


def test_density_against_ridge_rows(ctx, monkeypatch):
    import test_gpu_density as TDN
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_ridge(LP):
        TDN.test_loclinear_against_adjusted_rows(ctx, 0, 2000, 6, 3, 500, 12, 512)
    assert spy.n


def test_joint_against_ridge_rows(ctx, monkeypatch):
    import test_gpu_joint as TJ
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_ridge(LP):
        TJ.test_loclinear_against_adjusted_rows(ctx, 0, 2000, 6, 3, 257, 3, 64, True, None)
    assert spy.n


def test_draws_against_ridge_rows(ctx, monkeypatch):
    import test_gpu_draws as TDR
    case = (3, 64, 4096, 17, 1, 0, 0)
    assert case in TDR.TARGET_CASES
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_ridge(LP):
        TDR.test_targets_against_reference(ctx, *case)
    assert spy.n


def test_path_summary_against_ridge_rows(ctx):
    """tolerance t of the path summary against the summaries' reference on theta and weight of the adjust call with K = K_t under
    the same setting (test_gpu_summary.py's checks)"""
    import torch
    import test_gpu_summary as TS
    from abcsmc_amd import device
    N, M, P, B, Ks, kernel = 2000, 6, 3, 6, (16, 64, 257), 0
    X, Y = hetero_data(N, M, P, 77)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 5
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    truth = Y[rows].copy()
    with ctx.adjust_ridge(LP):
        g = _np(device.rank_targets_path_summary(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], probs=TS.PROBS,
                                                 truth=torch.tensor(truth), method=1, kernel=kernel, exclude=ex, ctx=ctx))
        assert ctx.last_ridge()[0].shape[0] == B * len(Ks)
    for t, K in enumerate(Ks):
        a = _adjust(ctx, F, F["model"], Td, K, LP, exclude=rows, kernel=kernel)
        off = _adjust(ctx, F, F["model"], Td, K, None, exclude=rows, kernel=kernel)
        assert not _same(a["theta"], off["theta"]) and _same(g["coef"][:, t], a["coef"])
        for b in range(B):
            rect = bool(a["status"][b] & 2)
            (TS._check_exact if rect else TS._check_bounds)(a["theta"][b:b + 1], a["weight"][b:b + 1], g["quant"][b:b + 1, t],
                                                           g["cdf"][b:b + 1, t], truth[b:b + 1])


# ---- composition ----------------------------------------------------------------------------------------------------------------
def test_with_transforms_and_the_variance_correction(ctx):
    """a log and a logit column, hcorr on: theta and hcoef against the reference of the composed definition (the ridge fit on
    the transformed scale, the second fit on its residuals, the rows carried back), with the same bound"""
    import torch
    from abcsmc_amd import device
    import test_gpu_transf as TT
    N, M, P, K, B = 2000, 6, 3, 500, 4
    X, Y = hetero_data(N, M, P, 21)
    Y = TT._unit(Y)
    F = _fit(ctx, X, Y, 3)
    kinds, lo, hi = TT._setting(P)
    assert "log" in kinds and "logit" in kinds
    rows = np.arange(B) * 13
    T = np.ascontiguousarray(X[rows])
    with ctx.param_transf(kinds, lo, hi):
        Yt = np.ascontiguousarray(device.param_transf(F["Yd"], ctx=ctx).cpu().numpy().T)      # the device's forward(Y), (N, P)
        g = _adjust(ctx, F, F["model"], T, K, L5, exclude=rows, hcorr=True)
    onscale = _adjust(ctx, F, F["model"], T, K, L5, exclude=rows, hcorr=True, Y=device.colmajor(Yt, DEV))     # the plain call on forward(Y)
    with ctx.param_transf(kinds, lo, hi):
        back = TT._back_rows(ctx, onscale["theta"])
    torch.cuda.synchronize()
    assert _same(g["coef"], onscale["coef"]) and _same(g["hcoef"], onscale["hcoef"]) and _same(g["pick"], onscale["pick"])
    assert np.array_equal(g["theta"], back)
    assert np.all(np.isfinite(g["hcoef"]))
    for b in (0, B - 1):
        _check_ref(F, T, onscale, b, F["ncomp"], 0, L5, "composed", Y=Yt, hcorr=True)


# ---- bad arguments --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from abcsmc_amd import _lib, abcutil
    Lb = _lib.lib()
    c = _lib.Context(0)
    n, nl, P = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
    assert Lb.abc_adjust_last_ridge(c.handle, None, 0, None, 0, C.byref(n), C.byref(nl), C.byref(P)) == 0
    assert (n.value, nl.value, P.value) == (0, 0, 0) and c.last_ridge()[0].shape == (0, 0) and c.adjust_ridge_unscored() == 0
    assert Lb.abc_adjust_last_ridge(c.handle, None, 0, None, 0, None, C.byref(nl), C.byref(P)) == INVALID
    X, Y = hetero_data(500, 4, 2, 1)
    good = (0.0, 0.25)
    c.set_adjust_ridge(good)
    kw = dict(max_comp=2, rule=0, ctx=c)
    want = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)
    assert c.last_ridge()[1].shape == (3, 2, 2)
    for bad in ((0.5, 0.1), (0.1, 0.1), (-1.0, 0.5), (0.0, float("nan")), (0.0, float("inf")), tuple(0.1 * i for i in range(9))):
        arr = np.asarray(bad, dtype=np.float64)
        assert Lb.abc_ctx_set_adjust_ridge(c.handle, arr.ctypes.data, arr.size) == INVALID, bad
        got = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)      # the previous setting is in force
        assert _same(got["coef"], want["coef"]) and c.last_ridge()[1].shape == (3, 2, 2), bad
    c.set_adjust_ridge(None)
    off = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, **kw)
    assert not _same(off["coef"], want["coef"])
    # rejection ignores the setting
    a = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[:3], 0.5, 50, **kw)
    b = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[:3], 0.5, 50, ridge=good, **kw)
    assert _same(a["quant"], b["quant"]) and "ridge_pick" not in b


# ---- usefulness -----------------------------------------------------------------------------------------------------------------
def test_the_choice_lowers_the_prediction_error(ctx):
    """test_ridge_cpu.py's data on the device: 100 left-out targets, K = 18 rows for 1 + 12 coefficients.  pred_error of
    cross_validate_pls(method="loclinear") is smaller with ridge = (0, 1e-3, 1e-2, 1e-1, 1) than without, for every parameter
    (the reference showed it for all twelve).  Measured: 0.14 to 0.33 with the choice, 0.23 to 0.86 without."""
    from abcsmc_amd import abcutil
    from test_ridge_cpu import LAMBDAS, USEFUL_COMP, USEFUL_K, usefulness_data
    X, Y, rows, _ = usefulness_data()
    kw = dict(max_comp=USEFUL_COMP, rule=0, ctx=ctx, method="loclinear")
    cv0 = abcutil.cross_validate_pls(X, Y, 100, USEFUL_K, seed=3, **kw)
    cv = abcutil.cross_validate_pls(X, Y, 100, USEFUL_K, seed=3, ridge=LAMBDAS, **kw)
    assert np.array_equal(cv["rows"], rows) and cv["ncomp"] == USEFUL_COMP
    print("usefulness (device): ncomp", cv["ncomp"], "pred_error with the choice", cv["pred_error"], "without", cv0["pred_error"])
    assert np.all(cv["pred_error"] < cv0["pred_error"])
    cvp = abcutil.cross_validate_pls_path(X, Y, 100, (USEFUL_K, 40), seed=3, ridge=LAMBDAS, **kw)
    assert np.allclose(cvp["pred_error"][0], cv["pred_error"], rtol=1e-12)
