"""Heteroscedastic variance correction of the local-linear adjustment (abc_ctx_set_adjust_hcorr, abc_adjust_last_hcorr,
abc_adjust_hcorr_skipped): the corrected rows and the second fit against the NumPy reference of the header's definition
(_hcorr_ref); a slot's bits alone, in a batch, through the host entry, through both gather paths and on a tolerance path; every
product under method 1 sees the corrected rows (the products' own tests run again under the setting, with their own bounds);
nothing else moves; rule 5 on the device; the refusals; and the correction recovers the local spread where the plain
adjustment does not.

The setting lives in the context the whole suite shares, so every test sets it inside Context.adjust_hcorr(...), which restores
what was there before."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _hcorr_ref as H
import _loclinear_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def hetero_data(N, M, P, seed, gamma=0.5):
    """parameters linear in the metrics plus noise whose log sd is linear in metric 0: continuous residuals"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, M))
    Y = X @ rng.normal(0.0, 1.0, (M, P)) + np.exp(gamma * X[:, :1]) * rng.standard_normal((N, P))
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _fit(ctx, X, Y, A):
    from test_gpu_adjust import _fit as fit
    return fit(ctx, X, Y, A)


def _adjust(ctx, F, model, T, K, exclude=None, kernel=0, on=True, Y=None, X=None, **kw):
    """device.rank_targets_adjust under the setting; returns the host arrays with hcoef = ctx.last_hcorr() added"""
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(T, DEV) if isinstance(T, np.ndarray) else T
    ex = torch.tensor(np.asarray(exclude)) if exclude is not None else None
    with ctx.adjust_hcorr(on):
        g = _np(device.rank_targets_adjust(F["Xd"] if X is None else X, model, F["A"], Td, K, F["Yd"] if Y is None else Y,
                                           exclude=ex, kernel=kernel, ctx=ctx, **kw))
        if on:
            g["hcoef"] = ctx.last_hcorr()
    return g


def _check_ref(F, T, g, b, nc, kernel, tag):
    """theta and hcoef within 1e-9 of each parameter column's range plus 100x what a relative 1e-15 perturbation of the scores
    changes in the reference (test_gpu_adjust.py's model); that widening term has to stay below 1e-8 of the range"""
    X, Y = F["X"], F["Y"]
    idx = g["idx"][b].astype(np.int64)
    S = R.scores(X[idx], F["mean"], F["sd"], F["R"], nc)
    o = R.scores(T[b], F["mean"], F["sd"], F["R"], nc)[0]
    ref = H.hcorr(g["dist"][b], S, o, Y[idx], kernel=kernel, A=F["A"])
    pert = H.hcorr(g["dist"][b], S * (1.0 + 1e-15 * np.random.default_rng(b).standard_normal(S.shape)), o, Y[idx],
                   kernel=kernel, A=F["A"])
    span = Y.max(axis=0) - Y.min(axis=0)
    assert g["rank"][b] == ref["rank"] == pert["rank"] and g["status"][b] == ref["status"], (tag, b)
    assert np.array_equal(g["weight"][b], ref["weight"]), (tag, b)
    assert not ref["skipped"].any(), (tag, b)
    for key in ("coef", "theta", "hcoef"):
        sens = np.abs(pert[key] - ref[key]).max(axis=0)
        err = np.abs(g[key][b] - ref[key]).max(axis=0)
        print("%s b=%d %s: err/range %.3g, widening/range %.3g" % (tag, b, key, (err / span).max(), (100.0 * sens / span).max()))
        assert np.all(100.0 * sens < 1e-8 * span), (tag, b, key, "the case breaks the condition: other data, not a wider bound")
        assert np.all(err <= 1e-9 * span + 100.0 * sens), (tag, b, key, (err / span).max())
    assert np.all(g["hcoef"][b][1 + nc:] == 0.0)
    return ref


# the issue's five shapes, and two more for the second-stage kernel's own branches: more than 256 entry groups of its (1 + nc) x P
# block (80 parameters, 12 components), and coefficients past its LDS budget (80 parameters, 52 components)
CASES = [(800, 5, 4, 16, 4, 0), (2000, 6, 3, 500, 12, 0), (5000, 8, 6, 4097, 3, 0), (1200, 4, 2, 64, 300, 0),
         (1500, 12, 80, 300, 3, 8), (1500, 16, 80, 300, 3, 12), (1500, 56, 80, 300, 2, 52)]


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
    for kernel in (0, 1):
        off = _adjust(ctx, F, model, T, K, exclude=rows, kernel=kernel, on=False)
        g = _adjust(ctx, F, model, T, K, exclude=rows, kernel=kernel)
        assert g["hcoef"].shape == (B, A + 1, P)
        for k in ("idx", "dist", "weight", "coef", "rank", "status"):
            assert _same(g[k], off[k]), k
        assert not _same(g["theta"], off["theta"])
        for b in sorted({0, B // 2, B - 1}):
            ref = _check_ref(F, T, g, b, nc, kernel, (N, M, P, K, B, kernel))
            assert np.abs(ref["theta"] - ref["plain"]).max() > 1e-3     # the correction does something here


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
    host = abcutil.particle_ranking_PLS_targets_adjust(X, Y, T, 0.5, K, exclude=rows, max_comp=3, rule=0, ctx=ctx, hcorr=True)
    assert host["ncomp"] == F["ncomp"] and getattr(ctx, "_hcorr", False) is False     # the wrapper restored the context
    for k in ("theta", "weight", "coef", "rank", "status", "hcoef"):
        assert _same(host[k], g[k]), k
    assert _same(host["hcoef"], ctx.last_hcorr())
    for b in (0, 5, 123, 299):
        one = _adjust(ctx, F, F["model"], T[b:b + 1], K, exclude=rows[b:b + 1])
        for k in ("idx", "theta", "weight", "coef", "hcoef"):
            assert _same(one[k][0], g[k][b]), (k, b)
    # strided and offset views of X, Y and the targets
    xbig = torch.full((M, N + 5), float("nan"), dtype=torch.float64, device=DEV)
    ybig = torch.full((P, N + 3), float("nan"), dtype=torch.float64, device=DEV)
    tbig = torch.full((M, B + 2), float("nan"), dtype=torch.float64, device=DEV)
    xbig[:, 1:N + 1], ybig[:, 2:N + 2], tbig[:, 1:B + 1] = F["Xd"], F["Yd"], device.colmajor(T, DEV)
    v = _adjust(ctx, F, F["model"], tbig[:, 1:B + 1], K, exclude=rows, X=xbig[:, 1:N + 1], Y=ybig[:, 2:N + 2])
    for k in ("idx", "theta", "weight", "coef", "hcoef"):
        assert _same(v[k], g[k]), k


def test_table_and_direct_gather_agree(tmp_path):
    """ABC_ADJ_GATHER=table / direct (ABC_DIAG=1), each in a fresh process: the same bits through both gather paths"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for path in ("table", "direct"):
        out = str(tmp_path / (path + ".npz"))
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "_hcorr_worker.py"), out], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, ABC_DIAG="1", ABC_ADJ_GATHER=path), cwd=root)
        assert p.returncode == 0, p.stderr[-3000:]
        res[path] = dict(np.load(out))
    assert len(res["table"]) == 10
    for k in res["table"]:
        assert _same(res["table"][k], res["direct"][k]), k
    assert np.all(np.isfinite(res["table"]["e_hcoef"]))


def _path_and_adjust(ctx, Ks, kernel):
    """the path under the setting (its outputs, with hcoef (B, T, A + 1, P) added), the same path without it, and the adjust call
    under the setting at every tolerance"""
    import torch
    from abcsmc_amd import device
    N, M, P, B = 3000, 6, 3, 5
    X, Y = hetero_data(N, M, P, 6)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 11
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    plain = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
    with ctx.adjust_hcorr(True):
        g = _np(device.rank_targets_path(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], exclude=ex, kernel=kernel, ctx=ctx))
        hc = ctx.last_hcorr()
    assert hc.shape == (B * len(Ks), F["A"] + 1, P) and np.all(np.isfinite(hc))
    g["hcoef"] = hc.reshape(B, len(Ks), F["A"] + 1, P)
    return g, plain, [_adjust(ctx, F, F["model"], Td, K, exclude=rows, kernel=kernel) for K in Ks]


@pytest.mark.parametrize("kernel", [0, 1])
def test_path_of_one_tolerance_is_the_adjustment(ctx, kernel):
    g, plain, adj = _path_and_adjust(ctx, (257,), kernel)
    for k in plain:                                                      # the path's own outputs do not move
        if isinstance(plain[k], np.ndarray):
            assert _same(plain[k], g[k]), k
    assert _same(g["coef"][:, 0], adj[0]["coef"]) and _same(g["hcoef"][:, 0], adj[0]["hcoef"])


@pytest.mark.parametrize("kernel", [0, 1])
def test_path_slots_are_the_adjustment_at_every_tolerance(ctx, kernel):
    """On a path of Ks = (64, 257, 1000) slot (b, t) of the hcoef record has the bits of the adjust call with K = K_t, at every
    tolerance: the path makes its second fits in that call's own order (its row chunks and its first fit over again).  The
    path's own coef is not part of the feature and keeps today's bits (asserted against the path without the setting): it sums
    over the row chunks of K_max (4 of 250 rows), so it has the adjust call's bits at tolerances 64 (inside the first chunk) and
    1000, and differs in the last bits at 257 (the adjust call: 2 chunks of 129), as the header says of the path."""
    Ks = (64, 257, 1000)
    g, plain, adj = _path_and_adjust(ctx, Ks, kernel)
    for k in plain:
        if isinstance(plain[k], np.ndarray):
            assert _same(plain[k], g[k]), k
    for t, K in enumerate(Ks):
        d = np.abs(g["hcoef"][:, t] - adj[t]["hcoef"]).max()
        print("kernel %d K_t = %d: hcoef same bits %s (largest difference %.3g), coef same bits %s" %
              (kernel, K, _same(g["hcoef"][:, t], adj[t]["hcoef"]), d, _same(g["coef"][:, t], adj[t]["coef"])))
        assert _same(g["hcoef"][:, t], adj[t]["hcoef"]), (kernel, K, d)
    for t in (0, 2):
        assert _same(g["coef"][:, t], adj[t]["coef"]), (kernel, Ks[t])
    assert np.allclose(g["coef"][:, 1], adj[1]["coef"], rtol=0, atol=1e-12 * np.abs(adj[1]["coef"]).max())


# ---- the products: their own tests, under the setting ------------------------------------------------------------------------
class _Spy:
    """records whether every device.rank_targets_adjust call made while a product's own test runs was corrected"""

    def __init__(self, monkeypatch, ctx):
        from abcsmc_amd import device
        self.n, real = 0, device.rank_targets_adjust

        def spy(*a, **kw):
            r = real(*a, **kw)
            h = ctx.last_hcorr()
            assert h.shape[0] == r["coef"].shape[0] and np.isfinite(h[:, 0]).any()
            with ctx.adjust_hcorr(False):
                off = real(*a, **kw)
            assert not _same(off["theta"].cpu().numpy(), r["theta"].cpu().numpy())
            assert _same(off["coef"].cpu().numpy(), r["coef"].cpu().numpy())
            self.n += 1
            return r
        monkeypatch.setattr(device, "rank_targets_adjust", spy)


@pytest.mark.parametrize("kernel,shape", [(0, (2000, 6, 3, 500, 12)), (1, (2000, 6, 3, 500, 12)), (0, (5000, 8, 6, 4097, 3))])
def test_summary_against_corrected_rows(ctx, monkeypatch, kernel, shape):
    """(the last shape: past the LDS path of the summaries)"""
    import test_gpu_summary as TS
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_hcorr(True):
        TS.test_loclinear_against_adjusted_rows(ctx, kernel, *shape)
    assert spy.n


@pytest.mark.parametrize("kernel", [0, 1])
def test_density_against_corrected_rows(ctx, monkeypatch, kernel):
    import test_gpu_density as TDN
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_hcorr(True):
        TDN.test_loclinear_against_adjusted_rows(ctx, kernel, 2000, 6, 3, 500, 12, 512)
    assert spy.n


@pytest.mark.parametrize("kernel", [0, 1])
def test_joint_against_corrected_rows(ctx, monkeypatch, kernel):
    import test_gpu_joint as TJ
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_hcorr(True):
        TJ.test_loclinear_against_adjusted_rows(ctx, kernel, 2000, 6, 3, 257, 3, 64, True, None)
    assert spy.n


@pytest.mark.parametrize("P,K,S,B,method,kernel,smooth", [(3, 64, 4096, 17, 1, 0, 0), (5, 257, 4096, 17, 1, 0, 1)])
def test_draws_against_reference(ctx, monkeypatch, P, K, S, B, method, kernel, smooth):
    """plain draws are rows of the corrected theta bit for bit, smoothed ones within test_gpu_draws.py's bounds"""
    import test_gpu_draws as TDR
    assert (P, K, S, B, method, kernel, smooth) in TDR.TARGET_CASES
    spy = _Spy(monkeypatch, ctx)
    with ctx.adjust_hcorr(True):
        TDR.test_targets_against_reference(ctx, P, K, S, B, method, kernel, smooth)
    assert spy.n


def test_summary_with_transforms_and_the_correction(ctx, monkeypatch):
    import test_gpu_summary as TS
    import test_gpu_transf as TT
    kinds, lo, hi = TT._setting(3)
    TT._unit_wl(TS, monkeypatch)
    spy = _Spy(monkeypatch, ctx)
    with ctx.param_transf(kinds, lo, hi), ctx.adjust_hcorr(True):
        TS.test_loclinear_against_adjusted_rows(ctx, 0, 2000, 6, 3, 500, 12)
    assert spy.n


@pytest.mark.parametrize("kernel", [0, 1])
def test_path_summary_against_corrected_rows(ctx, kernel):
    """tolerance t of the path summary against the summaries' reference on theta and weight of the adjust call with K = K_t
    under the same setting (test_gpu_summary.py's checks)"""
    import torch
    import test_gpu_summary as TS
    from abcsmc_amd import device
    N, M, P, B, Ks = 2000, 6, 3, 6, (16, 64, 257)
    X, Y = hetero_data(N, M, P, 77)
    F = _fit(ctx, X, Y, 3)
    rows = np.arange(B) * 5
    Td, ex = device.colmajor(X[rows], DEV), torch.tensor(rows)
    truth = Y[rows].copy()
    with ctx.adjust_hcorr(True):
        g = _np(device.rank_targets_path_summary(F["Xd"], F["model"], F["A"], Td, Ks, F["Yd"], probs=TS.PROBS,
                                                 truth=torch.tensor(truth), method=1, kernel=kernel, exclude=ex, ctx=ctx))
        assert ctx.last_hcorr().shape[0] == B * len(Ks)
    for t, K in enumerate(Ks):
        a = _adjust(ctx, F, F["model"], Td, K, exclude=rows, kernel=kernel)
        off = _adjust(ctx, F, F["model"], Td, K, exclude=rows, kernel=kernel, on=False)
        assert not _same(a["theta"], off["theta"])
        for b in range(B):
            rect = kernel == 1 or bool(a["status"][b] & 2)
            (TS._check_exact if rect else TS._check_bounds)(a["theta"][b:b + 1], a["weight"][b:b + 1], g["quant"][b:b + 1, t],
                                                           g["cdf"][b:b + 1, t], truth[b:b + 1])


# ---- nothing else moves -------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(ctx):
    import torch
    from abcsmc_amd import device
    N, M, P, K, B = 3000, 6, 3, 500, 5
    X, Y = hetero_data(N, M, P, 79)
    F = _fit(ctx, X, Y, 3)
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
        r["path"] = device.rank_targets_path(*args, (3, 64, K), F["Yd"], exclude=ex, ctx=ctx)
        r["path_summary"] = device.rank_targets_path_summary(*args, (3, 64, K), F["Yd"], exclude=ex, coef=False, fit=False, ctx=ctx)
        r["w_summary"] = device.weighted_summary(V, w, ctx=ctx)
        r["w_density"] = device.weighted_density(V, w, G=65, ctx=ctx)
        r["w_joint"] = device.weighted_joint(V, w, G=16, ctx=ctx)
        r["w_draws"] = device.weighted_draws(V, w, S=257, smooth=True, seed=5, ctx=ctx)
        return {k: _np(v) for k, v in r.items()}

    before, a_before = calls(), _adjust(ctx, F, F["model"], Td, K, exclude=rows, on=False)
    with ctx.adjust_hcorr(True):
        during = calls()
    a_during = _adjust(ctx, F, F["model"], Td, K, exclude=rows)
    a_after = _adjust(ctx, F, F["model"], Td, K, exclude=rows, on=False)
    for name in before:
        for k in before[name]:
            if isinstance(before[name][k], np.ndarray):
                assert _same(before[name][k], during[name][k]), (name, k)
    for k in a_before:
        assert _same(a_before[k], a_after[k]), k                         # off again: today's bits
        if k != "theta":
            assert _same(a_before[k], a_during[k]), k
    assert not _same(a_before["theta"], a_during["theta"])


# ---- rule 5 on the device -----------------------------------------------------------------------------------------------------
def test_rule5_on_the_device(ctx):
    from test_gpu_adjust import _with_nc
    N, M, P, B = 2000, 5, 4, 3
    X, Y = hetero_data(N, M, P, 13)
    X, Y = X.copy(), Y.copy()
    Y[:, 2] = 1.25                                                       # a constant column
    X[1:40] = X[0]                                                       # 40 identical rows: h == 0 for targets at them
    F = _fit(ctx, X, Y, 3)
    model = _with_nc(F, 3)
    T = np.ascontiguousarray(X[[0, 500, 900]])
    ctx.adjust_hcorr_skipped(reset=True)
    assert ctx.adjust_hcorr_skipped() == 0
    # a constant column: skipped for every target, the others corrected (target 0 sits on the duplicates: K = 300 reaches past them)
    K = 300
    off = _adjust(ctx, F, model, T, K, on=False)
    g = _adjust(ctx, F, model, T, K)
    assert np.isnan(g["hcoef"][:, 0, 2]).all() and np.all(g["hcoef"][:, 1:, 2] == 0.0)
    assert np.all(np.isfinite(g["hcoef"][:, :, [0, 1, 3]]))
    assert _same(g["theta"][:, :, 2], off["theta"][:, :, 2])
    for j in (0, 1, 3):
        assert not _same(g["theta"][:, :, j], off["theta"][:, :, j])
    assert ctx.adjust_hcorr_skipped() == B
    # duplicated rows, h == 0: the rectangular fallback without a kept pivot; alpha is the mean of 30 rows.  Column 2 (constant)
    # has zero residuals; the rest have none
    K = 30
    off = _adjust(ctx, F, model, T[:1], K, on=False)
    g = _adjust(ctx, F, model, T[:1], K)
    assert g["status"][0] & 2 and g["rank"][0] == 0
    ref = H.hcorr(g["dist"][0], np.zeros((K, 3)), np.zeros(3), Y[g["idx"][0].astype(np.int64)], A=F["A"])
    assert ref["skipped"].tolist() == np.isnan(g["hcoef"][0, 0]).tolist() == [False, False, True, False]
    assert _same(g["theta"][0][:, 2], off["theta"][0][:, 2]) and np.all(g["hcoef"][0, 1:] == 0.0)
    assert np.allclose(g["hcoef"][0, 0, [0, 1, 3]], ref["hcoef"][0, [0, 1, 3]], rtol=1e-12)
    assert ctx.adjust_hcorr_skipped() == B + 1
    # K = nc + 2: everything skipped, the rows are the plain adjustment's; K = nc + 3: nothing but the constant column
    off = _adjust(ctx, F, model, T[1:], 5, on=False)
    g = _adjust(ctx, F, model, T[1:], 5)
    assert np.isnan(g["hcoef"][:, 0]).all() and np.all(g["hcoef"][:, 1:] == 0.0) and _same(g["theta"], off["theta"])
    assert ctx.adjust_hcorr_skipped() == B + 1 + 2 * P
    g = _adjust(ctx, F, model, T[1:], 6)
    assert np.isnan(g["hcoef"][:, 0]).tolist() == [[False, False, True, False]] * 2
    assert ctx.adjust_hcorr_skipped(reset=True) == B + 1 + 2 * P + 2 and ctx.adjust_hcorr_skipped() == 0
    # a NaN parameter in one retained row (the farthest: weight 0) touches its own column only
    K = 200
    clean = _adjust(ctx, F, model, T[1:2], K)
    Yb = Y.copy()
    Yb[int(clean["idx"][0, K - 1]), 1] = np.nan
    from abcsmc_amd import device
    g = _adjust(ctx, F, model, T[1:2], K, Y=device.colmajor(Yb, DEV))
    off = _adjust(ctx, F, model, T[1:2], K, Y=device.colmajor(Yb, DEV), on=False)
    assert clean["weight"][0, K - 1] == 0.0
    assert np.isnan(g["hcoef"][0, 0]).tolist() == [False, True, True, False]
    for j in (0, 3):
        assert _same(g["theta"][0][:, j], clean["theta"][0][:, j]) and _same(g["hcoef"][0][:, j], clean["hcoef"][0][:, j])
    assert _same(g["theta"][0][:, 1], off["theta"][0][:, 1])
    assert ctx.adjust_hcorr_skipped(reset=True) == 1 + 2


# ---- bad arguments --------------------------------------------------------------------------------------------------------------
def test_arguments():
    from abcsmc_amd import _lib
    L = _lib.lib()
    c = _lib.Context(0)
    n, a1, P = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
    assert L.abc_adjust_last_hcorr(c.handle, None, 0, C.byref(n), C.byref(a1), C.byref(P)) == 0
    assert (n.value, a1.value, P.value) == (0, 0, 0) and c.last_hcorr().shape == (0, 0, 0)
    assert L.abc_ctx_set_adjust_hcorr(c.handle, 2) == INVALID and L.abc_ctx_set_adjust_hcorr(c.handle, -1) == INVALID
    assert c.adjust_hcorr_skipped() == 0
    assert L.abc_adjust_last_hcorr(c.handle, None, 0, None, C.byref(a1), C.byref(P)) == INVALID
    X, Y = hetero_data(500, 4, 2, 1)
    from abcsmc_amd import abcutil
    r = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[:3], 0.5, 50, max_comp=2, rule=0, ctx=c, hcorr=True)
    assert r["hcoef"].shape == (3, 3, 2)
    buf = np.full(18, -7.0)
    assert L.abc_adjust_last_hcorr(c.handle, None, 0, C.byref(n), C.byref(a1), C.byref(P)) == 0      # cap = 0: the counts only
    assert (n.value, a1.value, P.value) == (3, 3, 2)
    assert L.abc_adjust_last_hcorr(c.handle, buf.ctypes.data, 5, C.byref(n), C.byref(a1), C.byref(P)) == 0
    assert np.array_equal(buf[:5], r["hcoef"].reshape(-1)[:5]) and np.all(buf[5:] == -7.0)
    # rejection ignores the setting
    a = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[:3], 0.5, 50, max_comp=2, rule=0, ctx=c)
    b = abcutil.particle_ranking_PLS_targets_summary(X, Y, X[:3], 0.5, 50, max_comp=2, rule=0, ctx=c, hcorr=True)
    assert _same(a["quant"], b["quant"])


# ---- usefulness -----------------------------------------------------------------------------------------------------------------
def test_the_correction_recovers_the_local_spread(ctx):
    """test_hcorr_cpu.py's check on the device: N = 4000, K = 2000, 100 targets excluded from their own ranking.  The 90th
    percentile of |log(weighted sd of parameter 0's adjusted rows / exp(0.75 x_target))| is <= 0.1 with the correction and >= 0.3
    without; parameter 1's sd changes by less than 10 % at the median.  (The reference alone: 0.055, 0.500, 0.000.)"""
    from abcsmc_amd import abcutil
    from test_hcorr_cpu import usefulness_data, usefulness_figures
    X, Y, rows = usefulness_data()
    kw = dict(exclude=rows, max_comp=2, rule=0, ctx=ctx)
    off = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[rows], 0.5, 2000, **kw)
    on = abcutil.particle_ranking_PLS_targets_adjust(X, Y, X[rows], 0.5, 2000, hcorr=True, **kw)
    assert _same(on["weight"], off["weight"]) and _same(on["coef"], off["coef"]) and not np.isnan(on["hcoef"]).any()
    f_on, f_off, f_p1 = usefulness_figures(X, rows, on["theta"], off["theta"], on["weight"])
    print("usefulness (device): with %.3f without %.3f parameter 1 %.4f" % (f_on, f_off, f_p1))
    assert f_on <= 0.1 and f_off >= 0.3 and f_p1 < 0.1
    cv = abcutil.cross_validate_pls(X, Y, 100, 2000, seed=3, max_comp=2, rule=0, ctx=ctx, method="loclinear", statistic="median",
                                    coverage=True, hcorr=True)
    cv0 = abcutil.cross_validate_pls(X, Y, 100, 2000, seed=3, max_comp=2, rule=0, ctx=ctx, method="loclinear", statistic="median",
                                     coverage=True)
    assert not _same(cv["truth_cdf"], cv0["truth_cdf"])
