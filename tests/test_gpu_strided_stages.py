"""The stage entry points that take a leading dimension besides the statistics (tests/test_gpu_stats.py): projection distances,
the Wilcoxon reduction and the row gather, with ld > n (the gap rows [n, ld) NaN), base pointers 8 bytes off and ldx != ldy,
against the contiguous call (bit for bit) and the oracle.  Every caller in the package passes ld == n: these tests are what
holds a kernel to ldx / ldy / ldt."""
import numpy as np
import pytest

from test_gpu_stats import _dev_cols

pytestmark = pytest.mark.gpu


def _fma_dot(a, b):
    """m-ascending fma chain in float64 using exact arithmetic (as tests/test_gpu_parity.py)"""
    from fractions import Fraction
    s = 0.0
    for x, y in zip(a, b):
        s = float(Fraction(float(x)) * Fraction(float(y)) + Fraction(s))
    return s


def _data(n, M, P, seed):
    from abcsmc_amd import synthetic
    wl = synthetic.Workload(M, P, seed)
    X, Y = wl.rows(0, n)
    return np.asfortranarray(X), np.asfortranarray(Y), wl.observed()


def _model(gpu_ctx, X, Y, obs, A, simple, ntrain):
    """the device's model record (PLS under argmin PRESS, or the simple one) from contiguous statistics"""
    import torch
    from abcsmc_amd import _lib, device, sharded
    lib = _lib.lib()
    n, M = X.shape
    P = Y.shape[1]
    be = sharded.HipBackend("cuda:0", gpu_ctx)
    dX, dY, dobs = device.colmajor(X, "cuda:0"), device.colmajor(Y, "cuda:0"), device.colmajor(obs, "cuda:0")
    stats = be.zeros(be.stats_len(M, P))
    be.stats_shift(dX, dY, stats)
    be.stats_accumulate(dX, dY, 0, ntrain, stats)
    model = be.zeros(be.model_len(M, P, A) + 8)
    torch.cuda.synchronize()
    if simple:
        gpu_ctx.check(lib.abc_simple_model_dev(gpu_ctx.handle, stats.data_ptr(), dobs.data_ptr(), M, P, model.data_ptr()))
    else:
        be.pls_model(stats, dobs, M, P, A, _lib.RULE_MIN_PRESS, model)
    torch.cuda.synchronize()
    return model


def _distances(gpu_ctx, X, ld, off, M, P, A, model, simple):
    import torch
    from abcsmc_amd import _lib
    n = X.shape[0]
    tX, pX = _dev_cols(X, ld, off)
    dist = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.check(_lib.lib().abc_project_distance_dev(gpu_ctx.handle, pX, n, ld, M, P, A, model.data_ptr(), simple, dist.data_ptr()))
    torch.cuda.synchronize()
    d = dist.cpu().numpy()
    assert np.isnan(d[n:]).all(), "distances written past n"
    return d[:n]


@pytest.mark.parametrize("simple,A", [(1, 0), (0, 8), (0, 24), (0, 40)])
@pytest.mark.parametrize("n", [3000, 3001])
def test_project_distance_strided_and_offset(gpu_ctx, oracle, simple, A, n):
    """simple distances, A <= 16 (vector kernel), 17..32 (the matrix-pipe projection), > 32 (k_project_dist_wide): bit-identical
    to the contiguous call at ld = n + 1, n + 2, n + 64 and with the base 8 bytes off, and bit-exact against the oracle's
    projection given the device's model"""
    M, P = 48, 12
    X, Y, obs = _data(n, M, P, 3)
    model = _model(gpu_ctx, X, Y, obs, max(A, 1), simple, n // 2)
    m = model.cpu().numpy()
    base = _distances(gpu_ctx, X, n, 0, M, P, A, model, simple)
    mean, sd = m[4:4 + M], m[4 + M + P:4 + M + P + M]
    with np.errstate(invalid="ignore", divide="ignore"):
        zobs = np.where(sd == 0, 0.0, (obs - mean) / sd)
    if simple:
        ref = oracle.project_distance(X, mean, sd, np.eye(M), M, zobs)
    else:
        nc = int(m[0])
        off_R = 4 + 2 * (M + P) + M + A
        R = np.asfortranarray(m[off_R:off_R + M * A].reshape(A, M).T)
        so = np.array([_fma_dot(zobs, R[:, k]) for k in range(nc)])
        ref = oracle.project_distance(X, mean, sd, R, nc, so)
    assert np.array_equal(base, ref), "contiguous distances not bit-exact against the oracle"
    for ld, off in ((n + 1, 0), (n + 2, 0), (n + 64, 0), (n, 1), (n + 2, 1)):
        d = _distances(gpu_ctx, X, ld, off, M, P, A, model, simple)
        assert np.array_equal(d, base), (ld, off, int(np.sum(d != base)))


def _wilcoxon_counts(gpu_ctx, X, Y, model0, M, P, A, row_test, ldx, ldy, xoff, yoff):
    import torch
    from abcsmc_amd import _lib
    n = X.shape[0]
    model = model0.clone()
    tX, pX = _dev_cols(X, ldx, xoff)
    tY, pY = _dev_cols(Y, ldy, yoff)
    torch.cuda.synchronize()
    gpu_ctx.check(_lib.lib().abc_pls_wilcoxon_dev(gpu_ctx.handle, pX, pY, n, ldx, ldy, M, P, A, row_test, model.data_ptr()))
    torch.cuda.synchronize()
    m = model.cpu().numpy()
    L = _lib.lib().abc_model_len(M, P, A)
    return m[L - P:L].astype(int), int(m[0])


@pytest.mark.parametrize("row_test", ["odd", "half", "n"])
def test_wilcoxon_reduction_strided_and_offset(gpu_ctx, oracle, row_test):
    """the per-response component counts of abc_pls_wilcoxon_dev with ld > n (NaN gap rows), ldx != ldy and base pointers 8 bytes
    off equal the contiguous call's and the oracle's reduction on the device's own model"""
    n, M, P, A = 6001, 12, 5, 6
    X, Y, obs = _data(n, M, P, 11)
    rng = np.random.default_rng(7)
    Y = np.asfortranarray(Y + rng.normal(size=Y.shape) * Y.std(0) * 1.5)
    rt = {"odd": 3001, "half": n // 2, "n": n}[row_test]
    model0 = _model(gpu_ctx, X, Y, obs, A, False, rt)
    m0 = model0.cpu().numpy()
    base, nc = _wilcoxon_counts(gpu_ctx, X, Y, model0, M, P, A, rt, n, n, 0, 0)
    if rt < n:
        off_mean, off_sd = 4, 4 + M + P
        off_R = off_sd + (M + P) + M + A
        off_Q = off_R + M * A
        mean, sd = m0[off_mean:off_mean + M + P], m0[off_sd:off_sd + M + P]
        R = np.asfortranarray(m0[off_R:off_R + M * A].reshape(A, M).T)
        Q = np.asfortranarray(m0[off_Q:off_Q + P * A].reshape(A, P).T)
        with np.errstate(divide="ignore", invalid="ignore"):
            Zx = np.where(sd[:M] == 0, 0.0, (X[rt:] - mean[:M]) / sd[:M])
            Zy = np.where(sd[M:] == 0, 0.0, (Y[rt:] - mean[M:]) / sd[M:])
        _, o_wx = oracle.pls_optimal_components(Zx, Zy, R, Q, oracle.RULE_WILCOXON)
        assert np.array_equal(base, o_wx.astype(int)), (base, o_wx)
    for ldx, ldy, xoff, yoff in ((n + 1, n + 64, 0, 0), (n + 3, n + 2, 1, 0), (n, n + 1, 0, 1)):
        got, gnc = _wilcoxon_counts(gpu_ctx, X, Y, model0, M, P, A, rt, ldx, ldy, xoff, yoff)
        assert np.array_equal(got, base) and gnc == nc, (ldx, ldy, xoff, yoff, got, base)


def test_gather_rows_strided_with_foreign_indices(gpu_ctx):
    """theta[i, :] = Y[idx[i] - idx_base, :] for idx inside [idx_base, idx_base + n_local), exact; rows of theta whose index lies
    outside, and the gap rows [K, ldt) of theta, keep their sentinel; Y's gap rows [n_local, ldy) are NaN and never land"""
    import torch
    from abcsmc_amd import _lib
    rng = np.random.default_rng(5)
    n_local, P, K, base = 1001, 7, 777, 5000
    Y = np.asfortranarray(rng.normal(size=(n_local, P)))
    idx = rng.integers(0, base + n_local + 4000, size=K).astype(np.uint64)
    idx[:4] = [base, base + n_local - 1, base - 1, base + n_local]          # both ends of the range and one past either
    for ldy, ldt, yoff in ((n_local + 1, K + 3, 0), (n_local + 64, K + 64, 1), (n_local, K + 1, 1)):
        tY, pY = _dev_cols(Y, ldy, yoff)
        theta = torch.full((ldt * P + 1,), -7.5, dtype=torch.float64, device="cuda:0")
        didx = torch.from_numpy(idx.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        gpu_ctx.check(_lib.lib().abc_gather_rows_dev(gpu_ctx.handle, pY, n_local, ldy, P, didx.data_ptr(), K, base,
                                                     theta.data_ptr(), ldt))
        torch.cuda.synchronize()
        th = theta.cpu().numpy()
        assert th[ldt * P] == -7.5
        T = th[:ldt * P].reshape(P, ldt).T
        inside = (idx >= base) & (idx < base + n_local)
        assert inside[:2].all() and not inside[2:4].any() and inside.sum() > 50 and (~inside).sum() > 50
        assert np.array_equal(T[:K][inside], Y[(idx[inside] - base).astype(np.int64)]), (ldy, ldt, yoff)
        assert np.all(T[:K][~inside] == -7.5) and np.all(T[K:] == -7.5), (ldy, ldt, yoff)
