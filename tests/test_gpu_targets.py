"""Batched PLS ranking of one set against many observed targets (abc_rank_targets_dev, abc_particle_ranking_pls_targets):
every target's result must equal, bit for bit, the first K entries of the single-target abc_particle_ranking_pls."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = np.uint64(2 ** 64 - 1)


def _wl(M, P, N, seed=4242):
    from abcsmc_amd import synthetic
    wl = synthetic.Workload(M, P, seed)
    X, Y = wl.rows(0, N)
    return wl, X, Y


def _targets(wl, X, B, seed):
    """random vectors near the cloud, existing rows (distance 0), duplicates of an earlier target, far outside the cloud"""
    rng = np.random.default_rng(seed)
    N, M = X.shape
    fresh, _ = wl.rows_by_index((1 << 40) + seed * 100000 + np.arange(B))
    T = np.array(fresh)
    kinds = rng.integers(0, 4, size=B)
    for b in range(B):
        if kinds[b] == 1:
            T[b] = X[rng.integers(0, N)]
        elif kinds[b] == 2 and b > 0:
            T[b] = T[rng.integers(0, b)]
        elif kinds[b] == 3:
            T[b] = X.mean(axis=0) + 1e3 * X.std(axis=0) * rng.standard_normal(M)
    if B > 1:
        T[1] = X[N // 3]                   # one of each for certain
    if B > 2:
        T[2] = T[0]
    if B > 3:
        T[3] = X.mean(axis=0) - 1e4 * X.std(axis=0)
    return np.ascontiguousarray(T)


def _single(ctx, X, Y, t, f, A, rule, K):
    from abcsmc_amd import abcutil
    return abcutil.particle_ranking_PLS(X, Y, t, f, K=K, max_comp=A, rule=rule, details=True, ctx=ctx)


def _batched(ctx, X, Y, T, f, A, rule, K, exclude=None):
    from abcsmc_amd import abcutil
    return abcutil.particle_ranking_PLS_targets(X, Y, T, f, K, exclude=exclude, max_comp=A, rule=rule, details=True, ctx=ctx)


def _check_rows(tag, g, b, ref_idx, ref_dist, K):
    assert np.array_equal(g["idx"][b], ref_idx[:K]), (tag, b, K)
    assert np.array_equal(g["dist"][b].view(np.uint64), ref_dist[:K].view(np.uint64)), (tag, b, K)


# (N, M, P, A, rule, B, targets checked one by one): A = 0 -> min(M, P)
CASES = [
    (1000, 2, 2, 0, 0, 7, 7),
    (1000, 32, 16, 8, 1, 256, 24),
    (4097, 32, 16, 0, 1, 7, 7),          # odd N: the scores by the batched path's own kernel; 16 components
    (4097, 128, 2, 32, 0, 7, 7),         # odd N, 32 components
    (1000, 32, 16, 5, 0, 4096, 12),      # B = 4096 at small N; 5 components (not a fused-kernel width)
    (100000, 32, 16, 8, 1, 256, 16),     # the fused projection kernel (8 components, LDS loadings)
    (100000, 128, 16, 32, 0, 7, 7),      # ... on the fp64 matrix pipe (17..32 components)
    (100000, 2, 2, 0, 0, 7, 4),
    (20000, 40, 16, 40, 1, 7, 4),        # more than 32 components: read from the scores as needed
]


@pytest.mark.parametrize("N,M,P,A,rule,B,nchk", CASES)
def test_targets_equal_single_calls(gpu_ctx, N, M, P, A, rule, B, nchk):
    wl, X, Y = _wl(M, P, N)
    T = _targets(wl, X, B, seed=N + M + B)
    f = 0.5
    gpu_ctx.targets_fallbacks(reset=True)
    Ks = sorted({1, 17, N // 10, N})
    res = {K: _batched(gpu_ctx, X, Y, T, f, A, rule, K) for K in Ks}
    rng = np.random.default_rng(7)
    chk = sorted(set(range(min(4, B))) | set(rng.choice(B, size=min(nchk, B), replace=False).tolist()))
    for b in chk:
        s = _single(gpu_ctx, X, Y, T[b], f, A, rule, N)
        for K in Ks:
            assert res[K]["ncomp"] == s["ncomp"]
            _check_rows((N, M, P, A, rule, B), res[K], b, s["idx"], s["dist"], K)
    # ordinary targets (fresh draws of the model) at ordinary K never need the exact fallback
    if N > 4096:
        fresh, _ = wl.rows_by_index((1 << 41) + np.arange(min(B, 64)))
        fresh = np.ascontiguousarray(fresh)
        gpu_ctx.targets_fallbacks(reset=True)
        g17 = _batched(gpu_ctx, X, Y, fresh, f, A, rule, 17)
        _batched(gpu_ctx, X, Y, fresh, f, A, rule, N // 10)
        assert gpu_ctx.targets_fallbacks() == 0
        s = _single(gpu_ctx, X, Y, fresh[0], f, A, rule, 17)
        _check_rows("fresh", g17, 0, s["idx"], s["dist"], 17)


def test_targets_million_rows_sampled(gpu_ctx):
    N, M, P, A = 1000000, 32, 16, 8
    wl, X, Y = _wl(M, P, N, seed=99)
    T = _targets(wl, X, 16, seed=5)
    fresh, _ = wl.rows_by_index((1 << 41) + np.arange(64))
    gpu_ctx.targets_fallbacks(reset=True)
    _batched(gpu_ctx, X, Y, np.ascontiguousarray(fresh), 0.5, A, 1, 10000)
    assert gpu_ctx.targets_fallbacks() == 0               # ordinary targets: the batched selection alone
    g = _batched(gpu_ctx, X, Y, T, 0.5, A, 1, 10000)
    for b in (0, 1, 3, 9):
        s = _single(gpu_ctx, X, Y, T[b], 0.5, A, 1, 10000)
        _check_rows("1e6", g, b, s["idx"], s["dist"], 10000)


def test_targets_against_oracle(gpu_ctx, oracle):
    """the oracle's independent fit: indices exact given the model (the GPU's model fed to the oracle's projection and order)"""
    from abcsmc_amd import abcutil
    for (N, M, P, A) in [(3000, 32, 16, 8), (2001, 20, 4, 4)]:
        wl, X, Y = _wl(M, P, N, seed=17)
        T = _targets(wl, X, 5, seed=3)
        K = 50
        g = _batched(gpu_ctx, X, Y, T, 0.5, A, 0, K)
        for b in range(3):
            s = abcutil.particle_ranking_PLS(X, Y, T[b], 0.5, max_comp=A, rule=0, details=True, ctx=gpu_ctx)
            o = oracle.particle_ranking_pls(X, Y, T[b], 0.5, A, rule=0)
            assert g["ncomp"] == o["ncomp"]
            nc = o["ncomp"]
            z = np.where(s["sd"] == 0, 0.0, (T[b] - s["mean"]) / np.where(s["sd"] == 0, 1.0, s["sd"]))
            so = np.array([_fma_dot(z, s["R"][:, k]) for k in range(nc)])
            d = oracle.project_distance(X, s["mean"], s["sd"], s["R"], nc, so)
            order = oracle.ordered(d)
            assert np.array_equal(g["idx"][b], order[:K]), (N, b)
            assert np.array_equal(g["dist"][b], d[order[:K].astype(int)])
            assert np.allclose(g["dist"][b], o["dist"][g["idx"][b].astype(int)], rtol=1e-6)


def _fma_dot(a, b):
    from fractions import Fraction
    s = 0.0
    for x, y in zip(a, b):
        s = float(Fraction(float(x)) * Fraction(float(y)) + Fraction(s))
    return s


@pytest.fixture(scope="module")
def fitted(gpu_ctx):
    """one fitted set on the device, shared by the device-entry tests"""
    import torch
    from abcsmc_amd import _lib, abcutil, device
    N, M, P, A = 6001, 24, 6, 8
    wl, X, Y = _wl(M, P, N, seed=31)
    ctx = gpu_ctx
    g = abcutil.particle_ranking_PLS(X, Y, X[0], 0.5, max_comp=A, rule=0, details=True, ctx=ctx)
    dev = "cuda:0"
    L = _lib.lib()
    Xd, Yd = device.colmajor(X, dev), device.colmajor(Y, dev)
    stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=dev)
    model = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=dev)
    obs = torch.zeros(M, dtype=torch.float64, device=dev)
    ntr = int(np.floor(0.5 * N + 0.5))                # llround, as the single-target call splits
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
    ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, ntr, stats.data_ptr()))
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), obs.data_ptr(), M, P, A, 0, model.data_ptr()))
    torch.cuda.synchronize()
    T = _targets(wl, X, 9, seed=11)
    return dict(N=N, M=M, P=P, A=A, X=X, Y=Y, Xd=Xd, Yd=Yd, model=model, T=T, ctx=ctx, ncomp=g["ncomp"])


def test_device_entry_matches_host_call(fitted):
    """the device entry on the stage-built model equals the host drop-in (whose fit is the single call's)"""
    from abcsmc_amd import device
    import torch
    F = fitted
    K = 40
    h = _batched(F["ctx"], F["X"], F["Y"], F["T"], 0.5, F["A"], 0, K)
    Td = device.colmajor(F["T"], "cuda:0")
    idx, d, pm = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], post_mean=True)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy().astype(np.uint64), h["idx"])
    assert np.array_equal(d.cpu().numpy().view(np.uint64), h["dist"].view(np.uint64))
    assert np.array_equal(pm.cpu().numpy().view(np.uint64), h["post_mean"].view(np.uint64))


def test_device_entry_strided_and_offset(fitted):
    """ldx > N, ldt > B, sub-views; odd N and X one row off 16-byte alignment reach the batched path's own scores kernel"""
    import torch
    from abcsmc_amd import device
    F = fitted
    N, M, K = F["N"], F["M"], 33
    dev = "cuda:0"
    Td = device.colmajor(F["T"], dev)
    ref_idx, ref_d, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K)
    # X inside a wider buffer, one row in (8-byte offset: not 16-byte aligned), ldx = N + 7
    big = torch.full((M, N + 7), float("nan"), dtype=torch.float64, device=dev)
    big[:, 1:N + 1] = F["Xd"]
    Xv = big[:, 1:N + 1]
    tb = torch.full((M, 9 + 5), float("nan"), dtype=torch.float64, device=dev)
    tb[:, 2:11] = Td
    Tv = tb[:, 2:11]
    assert Xv.stride(0) == N + 7 and Tv.stride(0) == 14
    idx, d, _ = device.rank_targets(Xv, F["model"], F["A"], Tv, K)
    # and an aligned even-length prefix view through the fused kernel: N - 1 rows, ldx = N + 7
    big0 = torch.full((M, N + 7), float("nan"), dtype=torch.float64, device=dev)
    big0[:, :N] = F["Xd"]
    idx2, d2, _ = device.rank_targets(big0[:, :N - 1], F["model"], F["A"], Tv, K)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), ref_idx.cpu().numpy())
    assert np.array_equal(d.cpu().numpy().view(np.uint64), ref_d.cpu().numpy().view(np.uint64))
    # the prefix set: every target's rows equal the full set's with row N - 1 dropped
    ri, rd = ref_idx.cpu().numpy(), ref_d.cpu().numpy()
    i2, dd2 = idx2.cpu().numpy(), d2.cpu().numpy()
    for b in range(9):
        keep = ri[b] != N - 1
        n = int(keep.sum())
        assert np.array_equal(i2[b, :n], ri[b][keep]) and np.array_equal(dd2[b, :n], rd[b][keep])


def test_exclusion(gpu_ctx):
    N, M, P, A = 5000, 16, 4, 4
    wl, X, Y = _wl(M, P, N, seed=77)
    rows = np.array([5, 4999, 1234, 0, 77, 2500], dtype=np.int64)
    T = np.ascontiguousarray(X[rows])                  # each target equals its excluded row
    T[4] = X[9]                                        # ... except one: a row that is not excluded
    ex = rows.copy()
    ex[5] = -1                                         # and one excludes nothing
    for K in (1, 17, 600):
        g = _batched(gpu_ctx, X, Y, T, 0.5, A, 1, K, exclude=ex)
        for b in range(len(rows)):
            s = _single(gpu_ctx, X, Y, T[b], 0.5, A, 1, K + 1)
            keep = s["idx"] != np.uint64(ex[b]) if ex[b] >= 0 else np.ones(K + 1, bool)
            _check_rows("excl", g, b, s["idx"][keep], s["dist"][keep], K)
            assert ex[b] < 0 or np.uint64(ex[b]) not in g["idx"][b]


def test_fallback_branch_on_tied_rows(gpu_ctx):
    """many duplicated rows tied at the K-th distance, more than a candidate segment holds: the exact path runs, results
    still equal the single call"""
    N, M, P, A = 40000, 8, 3, 3
    wl, X, Y = _wl(M, P, N, seed=5)
    X = np.array(X)
    X[::2] = X[0]                                      # half of the rows are one point
    X = np.asfortranarray(X)
    T = np.ascontiguousarray(np.vstack([X[0], X[1], X[0] + 0.5 * X.std(axis=0)]))
    K = 3000
    gpu_ctx.targets_fallbacks(reset=True)
    g = _batched(gpu_ctx, X, Y, T, 0.5, A, 0, K)
    assert gpu_ctx.targets_fallbacks() >= 1
    for b in range(3):
        s = _single(gpu_ctx, X, Y, T[b], 0.5, A, 0, K)
        _check_rows("tied", g, b, s["idx"], s["dist"], K)
    # with exclusion too
    g = _batched(gpu_ctx, X, Y, T, 0.5, A, 0, K, exclude=np.array([0, 1, -1]))
    for b, e in enumerate([0, 1, -1]):
        s = _single(gpu_ctx, X, Y, T[b], 0.5, A, 0, K + 1)
        keep = s["idx"] != np.uint64(e) if e >= 0 else np.ones(K + 1, bool)
        _check_rows("tied-excl", g, b, s["idx"][keep], s["dist"][keep], K)


def test_post_mean(gpu_ctx):
    N, M, P, A = 8000, 32, 16, 8
    wl, X, Y = _wl(M, P, N, seed=8)
    T = _targets(wl, X, 20, seed=2)
    for K in (1, 17, 800):
        g = _batched(gpu_ctx, X, Y, T, 0.5, A, 1, K)
        for b in range(20):
            ref = np.mean(Y[g["idx"][b].astype(np.int64)].astype(np.longdouble), axis=0)
            tol = 1e-12 * np.abs(Y).max(axis=0)
            assert np.all(np.abs(g["post_mean"][b] - ref.astype(np.float64)) <= tol), (K, b)


def test_bad_arguments(gpu_ctx):
    from abcsmc_amd import _lib
    L = _lib.lib()
    N, M, P = 500, 6, 3
    wl, X, Y = _wl(M, P, N, seed=1)
    X, Y = np.asfortranarray(X), np.asfortranarray(Y)
    T = np.asfortranarray(X[:4])
    idx = np.empty(4 * N, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(B=4, K=10, ex=None, Tm=T, Xm=X, idx_=idx, Ym=Y):
        return L.abc_particle_ranking_pls_targets(gpu_ctx.handle, p(Xm), p(Ym), N, M, P, p(Tm), B, 0.5, 3, 0, p(ex), K, p(idx_),
                                                  None, None, None)

    def invalid(rc):
        assert rc == -1                                  # ABC_ERR_INVALID
        assert L.abc_last_error(gpu_ctx.handle)

    invalid(call(B=0))
    invalid(call(K=0))
    invalid(call(K=N + 1))
    invalid(call(K=N, ex=np.array([3, -1, -1, -1], dtype=np.int64).astype(np.uint64)))
    invalid(call(ex=np.array([N, -1, -1, -1], dtype=np.int64).astype(np.uint64)))
    invalid(call(Xm=None))
    invalid(call(idx_=None))
    Tn = T.copy()
    Tn[2, 1] = np.nan
    invalid(call(Tm=np.asfortranarray(Tn)))
    Ti = T.copy()
    Ti[0, 0] = np.inf
    invalid(call(Tm=np.asfortranarray(Ti)))
    # device entry: leading dimensions and null pointers
    import torch
    from abcsmc_amd import device
    Xd, Td = device.colmajor(X, "cuda:0"), device.colmajor(T, "cuda:0")
    model = torch.zeros(L.abc_model_len(M, P, 3), dtype=torch.float64, device="cuda:0")
    ib = torch.empty(4 * 10, dtype=torch.int64, device="cuda:0")
    dev = lambda ldx=N, ldt=4, Ym=None, ldy=N, pm=None, md=model, tg=Td: L.abc_rank_targets_dev(
        gpu_ctx.handle, Xd.data_ptr(), ldx, Ym, ldy, N, M, P, md.data_ptr() if md is not None else None, 3,
        tg.data_ptr() if tg is not None else None, ldt, 4, None, 10, ib.data_ptr(), None, pm)
    invalid(dev(ldx=N - 1))
    invalid(dev(ldt=3))
    invalid(dev(pm=ib.data_ptr()))                       # post_mean without Y
    invalid(dev(md=None))
    invalid(dev(tg=None))
    # each entry also refuses what the other one was shown to refuse above
    invalid(call(Tm=None))
    invalid(call(Ym=None))
    Yd = device.colmajor(Y, "cuda:0")
    invalid(dev(Ym=Yd.data_ptr(), ldy=N - 1, pm=ib.data_ptr()))
    dp = lambda t: t.data_ptr() if t is not None else None
    exd = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda:0")
    dev2 = lambda B=4, K=10, ex=None, Xm=Xd, idx_=ib, tg=Td, A=3: L.abc_rank_targets_dev(
        gpu_ctx.handle, dp(Xm), N, None, N, N, M, P, model.data_ptr(), A, tg.data_ptr(), 4, B, dp(ex), K, dp(idx_), None, None)
    invalid(dev2(B=0))
    invalid(dev2(K=0))
    invalid(dev2(K=N + 1))
    invalid(dev2(K=N, ex=exd([3, -1, -1, -1])))
    invalid(dev2(ex=exd([N, -1, -1, -1])))
    invalid(dev2(Xm=None))
    invalid(dev2(idx_=None))
    invalid(dev2(A=0))
    invalid(dev2(tg=device.colmajor(Tn, "cuda:0")))
    invalid(dev2(tg=device.colmajor(Ti, "cuda:0")))
    # the context stays usable
    g = _batched(gpu_ctx, X, Y, T, 0.5, 3, 0, 10)
    s = _single(gpu_ctx, X, Y, T[0], 0.5, 3, 0, 10)
    assert np.array_equal(g["idx"][0], s["idx"])


def test_cross_validate_pls(gpu_ctx):
    from abcsmc_amd import abcutil
    N, M, P = 20000, 32, 16
    wl, X, Y = _wl(M, P, N, seed=21)
    cv = abcutil.cross_validate_pls(X, Y, 64, 200, seed=3, training_fraction=0.5, max_comp=8, ctx=gpu_ctx)
    rows = cv["rows"]
    assert len(set(rows.tolist())) == 64 and np.array_equal(cv["theta"], Y[rows])
    raw = abcutil.particle_ranking_PLS_targets(X, Y, X[rows], 0.5, 200, exclude=rows, max_comp=8, details=True, ctx=gpu_ctx)
    assert np.array_equal(cv["post_mean"], raw["post_mean"])
    for b, r in enumerate(rows):
        assert np.uint64(r) not in raw["idx"][b]
    th = Y[rows]
    err = ((raw["post_mean"] - th) ** 2).sum(axis=0) / (64 * th.var(axis=0, ddof=1))
    assert np.allclose(cv["pred_error"], err, rtol=1e-12)
    assert np.all(cv["pred_error"] < 1.5)                # the metrics carry information about every parameter
