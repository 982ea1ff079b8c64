"""Highest-density intervals of the batched ranking (abc_rank_targets_hpd_dev, abc_particle_ranking_pls_targets_hpd,
abc_weighted_hpd*): the device against the NumPy reference of the header's definition (tests/_hpd_ref.py) built on the device's own
rows, adjusted values and weights; bit for bit wherever the weights are equal and on both paths, the summary call's bits at
(plo, phi) under any weights, within the summaries' accuracy contract of the long-double reference otherwise; batch, entry-point
and output-selection invariance; edges, argument errors and the cross-validation's two outputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _hpd_ref as H
import _summary_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MASS4 = (1e-6, 0.5, 0.95, 1 - 1e-9)
MASS16 = tuple(np.round(np.linspace(0.03, 0.99, 16), 3))
OUT = ("lo", "hi", "plo", "phi")


def _wl(M, P, N, seed):
    from abcsmc_amd import synthetic
    X, Y = synthetic.Workload(M, P, seed).rows(0, N)
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


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def _same(a, b):
    """the same bits up to the payload of a NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def _hpd(F, T, K, mass, method=0, kernel=0, exclude=None, adjust=(), dist=False, outputs=OUT):
    import torch
    from abcsmc_amd import device
    ex = torch.tensor(exclude, dtype=torch.int64) if exclude is not None else None
    return _np(device.rank_targets_hpd(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"], mass=mass, method=method,
                                       kernel=kernel, exclude=ex, dist=dist, adjust=adjust, outputs=outputs))


def _whpd(V, w, mass, outputs=OUT):
    import torch
    from abcsmc_amd import device
    return _np(device.weighted_hpd(torch.tensor(np.ascontiguousarray(V.T), device=DEV), None if w is None else torch.tensor(w),
                                   mass=mass, outputs=outputs))


def _check_exact(vals, wts, r, mass):
    """vals (B, K, P), wts (B, K) or None: the four outputs of every segment and mass bit for bit"""
    B, _, P = vals.shape
    for b in range(B):
        ref = H.hpd(vals[b], None if wts is None else wts[b], mass)
        for k, name in enumerate(OUT):
            assert _same(r[name][b], ref[k]), (name, b, r[name][b], ref[k])


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


# LDS path up to 8192 (one, two and three entries, around the work-group's 512 threads, the last sizes of the path), then the
# global path: one chunk plus one entry, exactly two chunks (one merge round), two chunks plus one entry (two merge rounds)
@pytest.mark.parametrize("K", [1, 2, 3, 5, 511, 512, 513, 8191, 8192, 8193, 16384, 16385])
def test_bit_exact_equal_weights(ctx, K):
    rng = np.random.default_rng(K)
    for P in (1, 3):
        V = rng.gamma(2.0, size=(K, P))
        for mass in (MASS4, MASS16):
            r = _whpd(V, None, mass)
            _check_exact(V[None], None, {k: r[k][None] for k in OUT}, mass)
        N = max(K + 40, 600)
        X, Y = _wl(5, P, N, 3 * K + P)
        F = _fit(ctx, X, Y, min(5, P))
        rows = np.arange(3) * 11
        for method, kernel in ((0, 0), (1, 1)):
            r3 = _hpd(F, X[rows], K, MASS4, method=method, kernel=kernel, exclude=rows, adjust=("theta", "weight") if method else ())
            vals = r3["theta"] if method else Y[r3["idx"].astype(np.int64)]
            _check_exact(vals, None, r3, MASS4)
            r16 = _hpd(F, X[rows], K, MASS16, method=method, kernel=kernel, exclude=rows)
            _check_exact(vals, None, r16, MASS16)
            r1 = _hpd(F, X[rows[:1]], K, MASS4, method=method, kernel=kernel, exclude=rows[:1])      # B = 1: target 0 alone
            for k in OUT:
                assert _same(r1[k][0], r3[k][0]), (k, method)


def test_forced_global_path_gives_the_lds_bits(ctx, tmp_path):
    """K = 4096 in a child process under ABC_DIAG=1 ABC_SUMMARY_PATH=global against this process on the LDS path: the same bits
    for equal and unequal weights (the sums' order depends on the tile only), and the reference's for the equal-weight matrix"""
    import _hpd_worker as Wk
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "global.npz")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_hpd_worker.py"), out], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, ABC_DIAG="1", ABC_SUMMARY_PATH="global"), cwd=root)
    assert p.returncode == 0, p.stderr[-3000:]
    glob = dict(np.load(out))
    lds = Wk.compute()
    assert sorted(glob) == sorted(lds) and len(lds) == 20
    for k in lds:
        assert _same(lds[k], glob[k]), k
    V, w = Wk.generic_inputs()
    ref = H.hpd(V, None, Wk.MASS)
    for k, name in enumerate(OUT):
        assert _same(glob["gen_eq_" + name], ref[k]), name
    assert not _same(glob["gen_eq_lo"], glob["gen_w_lo"])


def _summary_at(call, plo, phi):
    """the summary's quantiles at every segment's own (plo, phi): call(probs) -> quant (B, nq, P); plo, phi (B, nm, P).  The levels
    of all segments go into lists of at most 64, and each segment reads its own two."""
    B, nm, P = plo.shape
    lv = np.stack([plo, phi], axis=-1).reshape(-1)              # [b][m][j][end]
    got = np.empty((B, nm, P, 2))
    for s0 in range(0, lv.size, 64):
        q = call(tuple(lv[s0:s0 + 64]))
        for i in range(s0, min(s0 + 64, lv.size)):
            b, m, j, e = np.unravel_index(i, (B, nm, P, 2))
            got[b, m, j, e] = q[b, i - s0, j]
    return got[..., 0], got[..., 1]


def test_identity_with_the_summary_generic_weights(ctx):
    """unequal generic weights with zeros (n < K) and one weight of 1e-300 beside weights of order 1"""
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(8)
    for K in (700, 9000):
        V = rng.normal(size=(K, 2))
        w = rng.uniform(0.1, 1.0, size=K)
        w[::7] = 0.0
        w[3] = 1e-300
        h = abcutil.weighted_hpd(V, w, mass=(0.5, 0.95), ctx=ctx)
        qlo, qhi = _summary_at(lambda pr: abcutil.weighted_summary(V, w, probs=pr, ctx=ctx)["quant"][None], h["plo"][None], h["phi"][None])
        assert _same(qlo[0], h["lo"]) and _same(qhi[0], h["hi"]), K
        assert np.all(h["hi"] > h["lo"])


@pytest.mark.parametrize("case", ["epanechnikov", "row_weights", "hcorr", "logit"])
def test_identity_with_the_summary_rankings(ctx, case):
    from abcsmc_amd import abcutil
    X, Y = _wl(6, 3, 3000, 31)
    rows = np.arange(3) * 17
    kw = dict(method="loclinear", kernel="epanechnikov", exclude=rows, max_comp=3, rule=0, ctx=ctx)
    if case == "row_weights":
        kw.update(method="rejection", row_weights=np.random.default_rng(4).uniform(0.2, 1.0, size=3000))
    elif case == "hcorr":
        kw.update(hcorr=True)
    elif case == "logit":
        lo, hi = Y.min(axis=0), Y.max(axis=0)
        Y = np.ascontiguousarray(0.1 + 0.8 * (Y - lo) / (hi - lo))
        kw.update(transf=["logit", "none", "log"], bounds=np.array([[0.05, 1.0], [0.0, 1.0], [0.0, 1.0]]))
    K = 600
    h = abcutil.particle_ranking_PLS_targets_hpd(X, Y, X[rows], 0.5, K, mass=(0.5, 0.9), **kw)
    summ = lambda pr: abcutil.particle_ranking_PLS_targets_summary(X, Y, X[rows], 0.5, K, probs=pr, **kw)
    qlo, qhi = _summary_at(lambda pr: summ(pr)["quant"], h["plo"], h["phi"])
    assert _same(qlo, h["lo"]) and _same(qhi, h["hi"])
    assert np.all(np.isfinite(h["lo"])) and np.all(h["hi"] > h["lo"])
    plain = abcutil.particle_ranking_PLS_targets_hpd(X, Y, X[rows], 0.5, K, mass=(0.5, 0.9), exclude=rows, max_comp=3, rule=0, ctx=ctx)
    assert not _same(plain["lo"], h["lo"])                      # (the setting reached the values or the weights)


def test_unequal_weights_against_long_double(ctx):
    """Normal values, uniform(0.1, 1) weights, n in {64, 513, 1000}, 40 columns, masses 0.5 and 0.95: 240 intervals.
    |width_dev - width_ref| <= bound(lo) + bound(hi), _summary_ref.quantile_bound at the reference's plo and phi; each end under
    its own bound where the reference's winner beats its best candidate at another position (plo more than 1e-9 away) by more than a
    relative 1e-9 of its width; at most 10 % of the intervals may be left out by that rule.  Observed on an MI355X: worst width
    error 6.9e-4 of its bound, worst end error 1.5e-3 of its bound, 0 of 240 left out."""
    rng = np.random.default_rng(12)
    mass = (0.5, 0.95)
    worst_w = worst_e = 0.0
    out_n = tot = 0
    for n in (64, 513, 1000):
        V = rng.normal(size=(n, 40))
        w = rng.uniform(0.1, 1.0, size=n)
        r = _whpd(V, w, mass)
        lo, hi, plo, phi, margin = H.hpd(V, w, mass, np.longdouble)
        for j in range(40):
            for i in range(2):
                _, blo = R.quantile_bound(V[:, j], w, plo[i, j], n)
                _, bhi = R.quantile_bound(V[:, j], w, phi[i, j], n)
                ew = abs((r["hi"][i, j] - r["lo"][i, j]) - (hi[i, j] - lo[i, j]))
                worst_w = max(worst_w, ew / (blo + bhi))
                assert ew <= blo + bhi, (n, j, i, ew, blo + bhi)
                tot += 1
                if not margin[i, j] > 1e-9:
                    out_n += 1
                    continue
                el, eh = abs(r["lo"][i, j] - lo[i, j]), abs(r["hi"][i, j] - hi[i, j])
                worst_e = max(worst_e, el / blo, eh / bhi)
                assert el <= blo and eh <= bhi, (n, j, i, el, blo, eh, bhi, margin[i, j])
    print("hpd unequal weights: worst width error %.3g of its bound, worst end error %.3g of its bound, %d of %d left out"
          % (worst_w, worst_e, out_n, tot))
    assert tot == 240 and out_n <= 0.10 * tot, (out_n, tot)


def test_batch_entries_and_outputs(ctx):
    import torch
    from abcsmc_amd import abcutil, device
    X, Y = _wl(6, 3, 2500, 21)
    F = _fit(ctx, X, Y, 3)
    B, K = 5, 500
    rows = np.arange(B) * 13
    Td = device.colmajor(X[rows], DEV)
    for method in (0, 1):
        members = ("theta", "weight", "coef", "rank", "status") if method else ()
        full = _hpd(F, X[rows], K, MASS4, method=method, exclude=rows, dist=True, adjust=members)
        for b in range(B):
            one = _hpd(F, X[rows[b:b + 1]], K, MASS4, method=method, exclude=rows[b:b + 1])
            for k in OUT:
                assert _same(one[k][0], full[k][b]), (k, b, method)
        only = _hpd(F, X[rows], K, MASS4, method=method, exclude=rows, outputs=("hi",))
        assert _same(only["hi"], full["hi"]) and only["lo"] is None and only["plo"] is None and only["phi"] is None
        if method:
            a = _np(device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], exclude=torch.tensor(rows)))
            for k in ("idx", "dist") + members:
                assert np.array_equal(full[k], a[k], equal_nan=True), k
        else:
            idx, dist, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], exclude=torch.tensor(rows))
            torch.cuda.synchronize()
            assert np.array_equal(full["idx"], idx.cpu().numpy()) and np.array_equal(full["dist"], dist.cpu().numpy())
        host = abcutil.particle_ranking_PLS_targets_hpd(X, Y, X[rows], 0.5, K, mass=MASS4, method=("rejection", "loclinear")[method],
                                                        exclude=rows, max_comp=3, rule=0, ctx=ctx)
        assert np.array_equal(host["idx"].astype(np.int64), full["idx"])
        for k in OUT:
            assert _same(host[k], full[k]), (k, method)
    V = np.random.default_rng(2).normal(size=(3000, 4))
    w = np.random.default_rng(3).uniform(0, 1, size=3000)
    h = abcutil.weighted_hpd(V, w, mass=MASS16, ctx=ctx)
    d = _whpd(V, w, MASS16)
    for k in OUT:
        assert _same(h[k], d[k]), k


def test_edges(ctx):
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(6)
    # an inf in one column: that segment NaN, its neighbours exact
    V = rng.normal(size=(300, 3))
    V[17, 1] = np.inf
    r = _whpd(V, None, MASS4)
    assert all(np.isnan(r[k][:, 1]).all() and np.isfinite(r[k][:, [0, 2]]).all() for k in OUT)
    _check_exact(V[None], None, {k: r[k][None] for k in OUT}, MASS4)
    # signed zeros and repeated values
    V = np.round(rng.normal(size=(400, 2)) * 2.0) / 2.0
    V[::3, 0], V[1::3, 0] = -0.0, 0.0
    r = _whpd(V, None, MASS16)
    _check_exact(V[None], None, {k: r[k][None] for k in OUT}, MASS16)
    # all values equal: width 0 and the first valid candidate
    V = np.full((257, 1), -1.25)
    r = _whpd(V, None, (0.3, 0.9))
    assert _same(r["lo"], [[-1.25], [-1.25]]) and _same(r["hi"], r["lo"]) and _same(r["plo"], [[0.5 / 257], [0.5 / 257]])
    _check_exact(V[None], None, {k: r[k][None] for k in OUT}, (0.3, 0.9))
    # m beyond the knots' span: [u_0, u_{n-1}]
    V = rng.normal(size=(4, 2))
    r = _whpd(V, None, (0.75 + 1e-12, 0.99))
    for i in range(2):
        assert _same(r["lo"][i], V.min(axis=0)) and _same(r["hi"][i], V.max(axis=0))
        assert _same(r["plo"][i], [0.125, 0.125]) and _same(r["phi"][i], [0.875, 0.875])
    w = np.array([0.0, 2.0, 0.0, 0.0])                          # n = 1 under weights
    r = _whpd(V, w, (0.5,))
    assert _same(r["lo"][0], V[1]) and _same(r["hi"][0], V[1]) and _same(r["plo"][0], [0.5, 0.5]) and _same(r["phi"][0], [0.5, 0.5])
    # exclude applied: a target that is a row of the set does not retain itself
    X, Y = _wl(5, 2, 900, 2)
    F = _fit(ctx, X, Y, 2)
    rows = np.array([5, 77, 300])
    r = _hpd(F, X[rows], 120, MASS4, exclude=rows)
    free = _hpd(F, X[rows], 120, MASS4)
    assert all(rows[b] not in r["idx"][b] and rows[b] in free["idx"][b] for b in range(3))
    _check_exact(Y[r["idx"].astype(np.int64)], None, r, MASS4)


def test_argument_errors(ctx):
    import torch
    from abcsmc_amd import _lib, abcutil, device
    INVALID, UNSUPPORTED = -1, -4
    L = _lib.lib()
    N, M, P = 800, 5, 3
    X, Y = _wl(M, P, N, 4)
    F = _fit(ctx, X, Y, 3)
    T = X[:4]
    Xf, Yf, Tf = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(T)
    Yw = np.asfortranarray(np.random.default_rng(0).standard_normal((N, 1025)))
    Td = device.colmajor(T, DEV)
    hp = lambda v: v.ctypes.data_as(C.c_void_p) if v is not None else None
    dp = lambda t: t.data_ptr() if t is not None else None
    hbuf = np.empty(4 * 17 * 1025)
    dbuf = torch.empty(4 * 17 * 1025, dtype=torch.float64, device=DEV)
    ok = np.full(17, 0.5)
    keep = []

    def desc(buf, mass=ok, nm=1, outs=(1, 1, 1, 1)):
        keep.append(mass)                                       # (the descriptor holds an address only)
        return _lib.Hpd(mass.ctypes.data if mass is not None else None, nm, *[buf if o else None for o in outs])

    def host(hd, Ym=Yf, Pm=P, method=0, kernel=0):
        return L.abc_particle_ranking_pls_targets_hpd(ctx.handle, hp(Xf), hp(Ym), N, M, Pm, hp(Tf), 4, 0.5, 3, 0, None, 50, method, kernel,
                                                      None, None, None, C.byref(hd) if hd is not None else None, None)

    def dev(hd, Ym=F["Yd"], Pm=P, method=0, kernel=0):
        return L.abc_rank_targets_hpd_dev(ctx.handle, dp(F["Xd"]), N, dp(Ym), N, N, M, Pm, dp(F["model"]), 3, dp(Td), 4, 4, None, 50,
                                          method, kernel, None, None, None, C.byref(hd) if hd is not None else None)

    Vh = np.asfortranarray(np.random.default_rng(1).normal(size=(100, 2)))
    Vd = torch.tensor(np.ascontiguousarray(Vh.T), device=DEV)
    gen_host = lambda hd: L.abc_weighted_hpd(ctx.handle, hp(Vh), 100, 2, None, C.byref(hd) if hd is not None else None)
    gen_dev = lambda hd: L.abc_weighted_hpd_dev(ctx.handle, Vd.data_ptr(), 100, 100, 2, None, C.byref(hd) if hd is not None else None)

    def refused(rc, code):
        assert rc == code, rc
        assert L.abc_last_error(ctx.handle)

    for call, buf in ((host, hp(hbuf)), (dev, dbuf.data_ptr()), (gen_host, hp(hbuf)), (gen_dev, dbuf.data_ptr())):
        assert call(desc(buf)) == 0
        refused(call(None), INVALID)
        refused(call(desc(buf, nm=0)), INVALID)
        refused(call(desc(buf, nm=17)), INVALID)
        refused(call(desc(buf, outs=(0, 0, 0, 0))), INVALID)
        for bad in (np.nan, 0.0, 1.0, -0.1, 1.5, np.inf):
            refused(call(desc(buf, mass=np.array([0.5, bad]), nm=2)), INVALID)
        assert call(desc(buf, mass=np.array([0.5, np.nan]), nm=1)) == 0         # (only the first nm are read)
        assert call(desc(buf, nm=16)) == 0
        assert call(desc(buf, outs=(0, 1, 0, 0))) == 0
    for call in (host, dev):
        refused(call(desc(hp(hbuf) if call is host else dbuf.data_ptr()), method=2), INVALID)
        refused(call(desc(hp(hbuf) if call is host else dbuf.data_ptr()), kernel=2), INVALID)
    refused(host(desc(hp(hbuf)), Ym=Yw, Pm=1025), UNSUPPORTED)
    refused(dev(desc(dbuf.data_ptr()), Ym=device.colmajor(Yw, DEV), Pm=1025), UNSUPPORTED)
    for bad_w in (-np.ones(100), np.zeros(100), np.where(np.arange(100) == 7, np.nan, 1.0)):
        with pytest.raises(RuntimeError):
            abcutil.weighted_hpd(Vh, bad_w, ctx=ctx)
    torch.cuda.synchronize()
    r = abcutil.weighted_hpd(Vh, mass=(0.5,), ctx=ctx)                          # the context still works after the errors
    ref = H.hpd(Vh, None, (0.5,))
    assert all(_same(r[name], ref[k]) for k, name in enumerate(OUT))


def test_cross_validation(ctx):
    """cross_validate_pls(hpd=(0.5, 0.9)), N = 4000, 32 left-out rows, K = 300: hpd is the direct call's, hpd_coverage the count
    made again from hpd and the truths (exact; no calibration claim), every other key as without hpd"""
    from abcsmc_amd import abcutil
    X, Y = _wl(6, 3, 4000, 17)
    for method in ("rejection", "loclinear"):
        base = abcutil.cross_validate_pls(X, Y, 32, 300, seed=3, ctx=ctx, method=method, coverage=True)
        cv = abcutil.cross_validate_pls(X, Y, 32, 300, seed=3, ctx=ctx, method=method, coverage=True, hpd=(0.5, 0.9))
        assert sorted(cv) == sorted(list(base) + ["hpd", "hpd_coverage"])
        for k in base:
            assert np.array_equal(base[k], cv[k], equal_nan=True), k
        rows = cv["rows"]
        d = abcutil.particle_ranking_PLS_targets_hpd(X, Y, X[rows], 0.5, 300, mass=(0.5, 0.9), method=method, exclude=rows, ctx=ctx)
        assert cv["hpd"].shape == (32, 2, 2, 3) and cv["hpd_coverage"].shape == (2, 3)
        assert _same(cv["hpd"][:, :, 0, :], d["lo"]) and _same(cv["hpd"][:, :, 1, :], d["hi"])
        th = cv["theta"][:, None, :]
        inside = (cv["hpd"][:, :, 0, :] <= th) & (th <= cv["hpd"][:, :, 1, :])
        assert np.array_equal(cv["hpd_coverage"], inside.sum(axis=0) / 32.0)
        print(method, "hpd_coverage", cv["hpd_coverage"])
