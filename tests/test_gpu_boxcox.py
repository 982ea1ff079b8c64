"""GPU: the Box-Cox pre-pass of the metrics (abc_optimize_box_cox*, abc_box_cox*; the definition is in the header) against the
long-double reference of _boxcox_ref: the skew table to the fp64 parity bar, the pick, the transform to a bound worked out from
one-ulp log and expm1, the bit-for-bit promises, the status bits, the refusals, and the pipeline as a pure pre-pass."""
import ctypes as C
import functools

import numpy as np
import pytest

import _boxcox_ref as B
from test_boxcox_cpu import PICK_MARGIN, PICK_TABLES

pytestmark = pytest.mark.gpu

SKEW_BAR = 1e-9                     # |delta| <= 1e-9 max(1, |skew_ref|): the project's fp64 parity bar
NS = (2, 3, 63, 64, 65, 1000, 4097)
MS = (1, 5, 33)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _holder(X, pad=0):
    """numpy (n, M) -> an (M, n) column-major device holder whose row stride is n + pad"""
    import torch
    X = np.asarray(X, dtype=np.float64)
    n, M = X.shape
    buf = torch.full((M, n + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda:0")
    return buf[:, :n]


def _search(X, shift=None, grid_args=(-5, 5, 0.1), skew=True, pad=0, ctx=None):
    """device.optimize_box_cox with everything back on the host"""
    from abcsmc_amd import device
    r = device.optimize_box_cox(_holder(X, pad), *grid_args, shift=shift, skew=skew, ctx=ctx)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _reference(N, M, seed, grid_args=(-5, 5, 0.1)):
    X, shift = B.table(N, M, seed)
    return X, shift, B.search(X, B.grid(*grid_args), shift)


def _assert_skew(dev, ref, what):
    err = np.abs(dev.astype(B.LD) - ref) / np.maximum(1, np.abs(ref))
    worst = float(err.max())
    print("%s: max |skew - ref| / max(1, |ref|) = %.3g" % (what, worst))
    assert worst <= SKEW_BAR, what


# ---- skew table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
def test_skew_table_matches_the_long_double_reference(gpu_ctx, N, M):
    """every family (lognormal, gamma, uniform(0.5, 3), squared normal, near-constant at 1e-6, 1000 +- 50 with and without a shift
    of -900) sits among the first seven columns; the reference is made once per N for the widest table and shared"""
    X, shift, ref = _reference(N, max(MS), N)
    r = _search(X[:, :M], shift[:M])
    assert r["skew"].shape == (M, 100) and not r["status"].any()
    _assert_skew(r["skew"], ref["skew"][:M], "N=%d M=%d" % (N, M))


def test_skew_table_large(gpu_ctx):
    """more than one 2048-row chunk times 48: the second stage over the chunks; the 9-value grid, which holds lambda == 0"""
    args = (-2, 2, 0.5)
    X, shift, ref = _reference(100003, 3, 7, args)
    r = _search(X, shift, args)
    assert r["grid"].size == 9 and r["grid"][4] == 0.0
    _assert_skew(r["skew"], ref["skew"], "N=100003 M=3 L=9")
    assert np.array_equal(r["pick"], ref["pick"])


# ---- pick ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,seed", PICK_TABLES)
def test_pick_equals_the_reference_pick(gpu_ctx, N, M, seed):
    """every column of these tables has a reference margin above 2e-9 (test_boxcox_cpu checks that without a GPU), so none is skipped"""
    X, shift, ref = _reference(N, M, seed)
    assert min(B.margin(ref["skew"][j]) for j in range(M)) > PICK_MARGIN
    r = _search(X, shift)
    assert np.array_equal(r["pick"], ref["pick"])
    assert _same(r["lam"], ref["lam"]) and _same(r["lam"], r["grid"][r["pick"]])
    assert _same(r["skew_best"], r["skew"][np.arange(M), r["pick"]])
    _assert_skew(r["skew_best"], ref["skew_best"], "best skew")


def test_pick_on_a_near_tie_is_one_of_the_two(gpu_ctx):
    x, g = B.near_tie_column()
    sk, _ = B.skew_table(x, g)
    r = _search(x[:, None], None, (-1.75, 1.75, 0.5))
    assert _same(r["grid"], g)
    assert int(r["pick"][0]) in B.near_tie_indices(sk)
    _assert_skew(r["skew"][0], sk, "near tie")


# ---- apply ----------------------------------------------------------------------------------------------------------------------------
def _assert_apply(y, x, lam, shift, what):
    """|y - y_ref| <= 8 (|lambda l| + 2) 2^-53 |y_ref|: one-ulp log and expm1, the amplification a e^a / (e^a - 1) <= |a| + 1 of the
    logarithm's error, and a margin of 8; non-finite reference values must match exactly"""
    worst = 0.0
    for j in range(x.shape[1]):
        ref, a = B.apply(x[:, j], lam[j], shift[j])
        with np.errstate(over="ignore"):
            ref64 = ref.astype(np.float64)                                  # past fp64's range: +-inf, which the device must give too
        fin, inf = np.isfinite(ref64), np.isinf(ref64)
        assert np.array_equal(np.isnan(y[:, j]), np.isnan(ref64)), (what, j)
        assert np.array_equal(y[inf, j], ref64[inf]), (what, j)
        with np.errstate(all="ignore"):
            err = np.abs(y[fin, j].astype(B.LD) - ref[fin])
            bound = 8 * (a[fin] + 2) * B.LD(2.0 ** -53) * np.abs(ref[fin])
            ulps = err / (B.LD(2.0 ** -53) * np.abs(ref[fin]))
        bad = err > bound
        assert not bad.any(), (what, j, float(lam[j]), x[fin, j][bad][:3], y[fin, j][bad][:3], ref[fin][bad][:3])
        if ulps.size:
            worst = max(worst, float(np.nanmax(np.where(np.abs(ref[fin]) > 0, ulps / (a[fin] + 2), 0))))
    print("%s: worst error %.3g x (|lambda l| + 2) 2^-53 |y| (bound 8)" % (what, worst))


def test_apply_matches_the_long_double_reference(gpu_ctx):
    from abcsmc_amd import device
    g = np.random.default_rng(21)
    lam = np.array([-5.0, -0.5, 0.0, float(np.float32(0.1)), 1.0, 4.9000001475, 7.450580596923828e-08])
    shift = np.array([0.0, 0.0, 0.0, 2.5, 0.0, 0.0, -900.0])
    n, M = 1001, lam.size
    x = np.exp(g.uniform(-3, 3, (n, M)))
    x[:, 3] = g.uniform(-2.0, 5.0, n)                                       # with its shift: (0.5, 7.5)
    x[:, 6] = 1000.0 + 50.0 * g.uniform(-1, 1, n)
    x[0, :3] = 1.0                                                          # l == 0
    y = device.to_numpy(device.box_cox(_holder(x), lam, shift))
    _assert_apply(y, x, lam, shift, "apply")


def test_apply_pinned_values(gpu_ctx):
    from abcsmc_amd import device
    nan, inf = np.nan, np.inf
    col = np.array([0.0, -0.0, -1.0, inf, -inf, nan, 1.0, 2.0, 5e-324, 1.7e308])
    lam = np.array([-2.0, 0.0, 2.0, 0.5])
    x = np.stack([col] * lam.size, axis=1)
    y = device.to_numpy(device.box_cox(_holder(x), lam))
    #                 z = 0   -0     <0   +inf  -inf  NaN   1    (finite ones are checked against the reference below)
    assert list(y[:2, 0]) == [-inf, -inf] and y[3, 0] == 0.5              # lambda < 0: -inf at 0; the limit -1 / lambda at +inf
    assert list(y[:2, 1]) == [-inf, -inf] and y[3, 1] == inf              # lambda == 0: log
    assert list(y[:2, 2]) == [-0.5, -0.5] and y[3, 2] == inf              # lambda > 0: -1 / lambda at 0
    assert np.isnan(y[[2, 4, 5], :]).all() and np.all(y[6, :] == 0.0)
    _assert_apply(y, x, lam, np.zeros(lam.size), "pinned")


def test_apply_in_place_strided_and_target_block(gpu_ctx):
    import torch
    from abcsmc_amd import device
    X, shift, _ = _reference(1000, 5, 1000)
    lam = np.array([-1.5, 0.0, 0.5, 2.0, float(np.float32(0.1))])
    plain = device.box_cox(_holder(X), lam, shift)
    assert plain.is_contiguous()
    h = _holder(X, pad=7)
    assert device.box_cox(h, lam, shift, out=h) is h                        # in place, ldx = ldo = n + 7
    assert _same(h.cpu().numpy(), plain.cpu().numpy())
    assert torch.isnan(h._base[:, 1000:]).all()                             # nothing written past the rows
    o = _holder(np.zeros_like(X), pad=3)
    device.box_cox(_holder(X), lam, shift, out=o)                           # ldo > n
    assert _same(o.cpu().numpy(), plain.cpu().numpy())
    T = _holder(X[100:109], pad=5)                                          # a B x M block of targets, ldt > B
    t = device.box_cox(T, lam, shift)
    assert _same(t.cpu().numpy(), plain[:, 100:109].contiguous().cpu().numpy())
    _assert_apply(device.to_numpy(plain), X, lam, shift, "table")


# ---- bits ------------------------------------------------------------------------------------------------------------------------------
KEYS = ("lam", "skew_best", "pick", "status", "skew")


def test_bits_repeat_alone_stride_entry_and_outputs(gpu_ctx):
    from abcsmc_amd import device
    N, M = 4097, 5
    X, shift, _ = _reference(N, max(MS), N)
    X, shift = X[:, :M], shift[:M]
    a = _search(X, shift)
    b = _search(X, shift)
    for k in KEYS:
        assert _same(a[k], b[k]), ("repeat", k)
    for j in range(M):                                                      # a column alone and among others
        one = _search(X[:, j:j + 1], shift[j:j + 1])
        for k in KEYS:
            assert _same(one[k][0], a[k][j]), ("alone", j, k)
    p = _search(X, shift, pad=7)                                            # ldx = N + 7
    for k in KEYS:
        assert _same(a[k], p[k]), ("ldx", k)
    h = gpu_ctx.optimize_box_cox(np.asfortranarray(X), B.grid(), shift, skew=True)   # the host entry
    for k in KEYS:
        assert _same(a[k], h[k]), ("host entry", k)
    h2 = gpu_ctx.optimize_box_cox(np.asfortranarray(X), B.grid(), shift, skew=False)
    n = _search(X, shift, skew=False)                                       # without the skew table
    assert n["skew"] is None and h2["skew"] is None
    for k in KEYS[:-1]:
        assert _same(a[k], n[k]) and _same(a[k], h2[k]), ("no skew", k)
    only = np.empty(M)                                                      # lambda alone, every other member NULL
    from abcsmc_amd import _lib
    out = _lib.BoxCoxOut(only.ctypes.data, None, None, None, None)
    Xf, g = np.asfortranarray(X), B.grid()
    gpu_ctx.check(_lib.lib().abc_optimize_box_cox(gpu_ctx.handle, Xf.ctypes.data, N, M, shift.ctypes.data, g.ctypes.data, g.size,
                                                  C.byref(out)))
    assert _same(only, a["lam"])


# ---- status bits -----------------------------------------------------------------------------------------------------------------------
def test_status_bad_constant_and_single_row(gpu_ctx):
    X, shift, ref = _reference(65, 5, 65)
    X = X.copy()
    X[17, 1] = 0.0                                                          # a zero
    X[:, 3] = 42.0                                                          # a constant column
    r = _search(X, shift)
    assert list(r["status"]) == [0, B.BAD, 0, B.CONSTANT, 0]
    assert r["lam"][1] == 1.0 and r["pick"][1] == -1 and np.isnan(r["skew"][1]).all() and np.isnan(r["skew_best"][1])
    assert r["pick"][3] == 0 and r["lam"][3] == -5.0 and np.all(r["skew"][3] == 0) and r["skew_best"][3] == 0
    for j in (0, 2, 4):                                                     # the neighbours of a refused column keep their bits' worth
        _assert_skew(r["skew"][j], ref["skew"][j], "beside a bad column, j=%d" % j)
    for bad in (-1.0, np.nan, np.inf):
        Y = X.copy()
        Y[3, 0] = bad
        assert _search(Y, shift)["status"][0] == B.BAD
    Z = X.copy()
    Z[17, 1] = 1.0
    assert _search(Z, shift + np.array([0, -1.0, 0, 0, 0]))["status"][1] == B.BAD      # ... <= 0 after the shift
    one = _search(np.array([[3.0, 0.5]]))                                   # N = 1
    assert list(one["status"]) == [B.CONSTANT] * 2 and list(one["pick"]) == [0, 0] and np.all(one["skew"] == 0)


def test_status_overflow_at_the_far_lambda(gpu_ctx):
    """logs from -133 to +267 about their mean: exp(5 x 267) is past fp64, the far grid values are skipped (bit 2), and the pick is
    the reference's rule over the values that are finite, which agree with the long-double reference"""
    l = -200.0 + 400.0 * (np.arange(64) / 63.0) ** 2
    x = np.exp(l)[:, None]
    g = B.grid()
    r = _search(x)
    sk = r["skew"][0]
    fin = np.isfinite(sk)
    assert r["status"][0] == B.SKIPPED and 10 < fin.sum() < 100 and not fin[0] and not fin[-1]
    assert int(r["pick"][0]) == B.pick(sk)[0] and fin[r["pick"][0]] and r["lam"][0] == g[r["pick"][0]]
    ref, _ = B.skew_table(x[:, 0], g)
    _assert_skew(sk[fin], ref[fin], "finite part")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    ctx = gpu_ctx
    N, M = 100, 3
    X = np.asfortranarray(np.random.default_rng(5).uniform(1, 2, (N, M)))
    d = _holder(X)
    g = B.grid()
    lam = torch.empty(M, dtype=torch.float64, device="cuda:0")
    out = _lib.BoxCoxOut(lam.data_ptr(), None, None, None, None)
    lam_h, hout = np.ones(M), np.empty(M)
    hstruct = _lib.BoxCoxOut(hout.ctypes.data, None, None, None, None)
    ok_shift, bad_shift = np.zeros(M), np.array([0.0, np.nan, 0.0])
    bad_grid, bad_lam = g.copy(), np.array([1.0, np.inf, 0.0])
    bad_grid[7] = np.nan
    y = np.empty((N, M), order="F")

    def refused(rc, code, *words):
        msg = L.abc_last_error(ctx.handle).decode()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    INV, UNS = -1, -4                                                       # ABC_ERR_INVALID, ABC_ERR_UNSUPPORTED
    P, gp, sp = d.data_ptr(), g.ctypes.data, ok_shift.ctypes.data
    sd = lambda *a: L.abc_optimize_box_cox_dev(ctx.handle, *a)
    refused(sd(None, N, N, M, sp, gp, g.size, C.byref(out)), INV, "abc_optimize_box_cox_dev", "null")
    refused(sd(P, N, N, M, sp, None, g.size, C.byref(out)), INV, "abc_optimize_box_cox_dev", "null")
    refused(sd(P, N, N, M, sp, gp, g.size, None), INV, "abc_optimize_box_cox_dev", "null")
    refused(sd(P, N, N, M, sp, gp, g.size, C.byref(_lib.BoxCoxOut(None, None, None, None, None))), INV, "abc_optimize_box_cox_dev", "out->lambda")
    refused(sd(P, N, 0, M, sp, gp, g.size, C.byref(out)), INV, "abc_optimize_box_cox_dev", "N = 0")
    refused(sd(P, N, N, 0, sp, gp, g.size, C.byref(out)), INV, "abc_optimize_box_cox_dev", "M = 0")
    refused(sd(P, N - 1, N, M, sp, gp, g.size, C.byref(out)), INV, "abc_optimize_box_cox_dev", "ldx 99 < N 100")
    refused(sd(P, N, N, M, sp, gp, 0, C.byref(out)), INV, "abc_optimize_box_cox_dev", "L = 0", "1..512")
    refused(sd(P, N, N, M, sp, gp, 513, C.byref(out)), INV, "abc_optimize_box_cox_dev", "L = 513")
    refused(sd(P, N, N, M, sp, bad_grid.ctypes.data, g.size, C.byref(out)), INV, "abc_optimize_box_cox_dev", "grid[7]")
    refused(sd(P, N, N, M, bad_shift.ctypes.data, gp, g.size, C.byref(out)), INV, "abc_optimize_box_cox_dev", "shift[1]")
    refused(sd(P, 2 ** 32, 2 ** 32, M, sp, gp, g.size, C.byref(out)), UNS, "abc_optimize_box_cox_dev", "2^32")
    sh = lambda *a: L.abc_optimize_box_cox(ctx.handle, *a)
    refused(sh(None, N, M, sp, gp, g.size, C.byref(hstruct)), INV, "abc_optimize_box_cox:", "null")
    refused(sh(X.ctypes.data, 0, M, sp, gp, g.size, C.byref(hstruct)), INV, "abc_optimize_box_cox:", "N = 0")
    refused(sh(X.ctypes.data, N, M, sp, gp, 600, C.byref(hstruct)), INV, "abc_optimize_box_cox:", "L = 600")
    refused(sh(X.ctypes.data, N, M, bad_shift.ctypes.data, gp, g.size, C.byref(hstruct)), INV, "abc_optimize_box_cox:", "shift[1]")
    ad = lambda *a: L.abc_box_cox_dev(ctx.handle, *a)
    lp = lam_h.ctypes.data
    refused(ad(None, N, N, M, lp, None, P, N), INV, "abc_box_cox_dev", "null")
    refused(ad(P, N, N, M, None, None, P, N), INV, "abc_box_cox_dev", "null")
    refused(ad(P, N, N, M, lp, None, None, N), INV, "abc_box_cox_dev", "null")
    refused(ad(P, N, 0, M, lp, None, P, N), INV, "abc_box_cox_dev", "n = 0")
    refused(ad(P, N, N, 0, lp, None, P, N), INV, "abc_box_cox_dev", "M = 0")
    refused(ad(P, N - 1, N, M, lp, None, P, N), INV, "abc_box_cox_dev", "ldx 99 < n 100")
    refused(ad(P, N, N, M, lp, None, P, N - 1), INV, "abc_box_cox_dev", "ldo 99 < n 100")
    refused(ad(P, N, N, M, bad_lam.ctypes.data, None, P, N), INV, "abc_box_cox_dev", "lambda[1]")
    refused(ad(P, N, N, M, lp, bad_shift.ctypes.data, P, N), INV, "abc_box_cox_dev", "shift[1]")
    refused(ad(P, 2 ** 32, 2 ** 32, M, lp, None, P, 2 ** 32), UNS, "abc_box_cox_dev", "2^32")
    ah = lambda *a: L.abc_box_cox(ctx.handle, *a)
    refused(ah(None, N, M, lp, None, y.ctypes.data), INV, "abc_box_cox:", "null")
    refused(ah(X.ctypes.data, N, M, bad_lam.ctypes.data, None, y.ctypes.data), INV, "abc_box_cox:", "lambda[1]")
    refused(ah(X.ctypes.data, N, 0, lp, None, y.ctypes.data), INV, "abc_box_cox:", "M = 0")
    ctx.synchronize()
    assert _same(d.cpu().numpy(), np.ascontiguousarray(X.T))                # the refused calls left the table alone
    ctx.check(sd(P, N, N, M, sp, gp, g.size, C.byref(out)))                 # and the context still works
    assert np.isfinite(lam.cpu().numpy()).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_pipeline_is_a_pure_pre_pass(gpu_ctx):
    """metrics exp(linear in the parameters + noise): the search finds the logarithm (lambda within one grid step of 0) for every
    column, and ranking on box_cox_metrics' table and targets has the bits of ranking on arrays transformed by abcutil.box_cox"""
    from abcsmc_amd import abcutil
    g = np.random.default_rng(77)
    N, M, P, Bt, K = 4000, 5, 3, 4, 100
    Y = g.standard_normal((N, P))
    W = g.uniform(0.2, 0.5, (P, M)) * g.choice([-1.0, 1.0], (P, M))
    c = g.uniform(-1, 3, M)
    X = np.exp(Y @ W + 0.2 * g.standard_normal((N, M)) + c)
    T = np.exp(g.standard_normal((Bt, P)) @ W + c)
    m = abcutil.box_cox_metrics(X, T, ctx=gpu_ctx)
    print("lambda:", m["lam"])
    assert not m["status"].any() and np.all(np.abs(m["lam"]) <= 0.1 + 1e-6)      # one grid step (the grid's own rounding: 1.5e-7)
    assert m["X"].shape == X.shape and m["targets"].shape == T.shape
    Xt, Tt = abcutil.box_cox(X, m["lam"], m["shift"], ctx=gpu_ctx), abcutil.box_cox(T, m["lam"], m["shift"], ctx=gpu_ctx)
    assert _same(Xt, m["X"]) and _same(Tt, m["targets"])
    a = abcutil.particle_ranking_PLS_targets(m["X"], Y, m["targets"], 0.5, K, details=True, ctx=gpu_ctx)
    b = abcutil.particle_ranking_PLS_targets(Xt, Y, Tt, 0.5, K, details=True, ctx=gpu_ctx)
    for k in ("idx", "dist", "post_mean"):
        assert _same(a[k], b[k]), k
    assert a["ncomp"] == b["ncomp"]
    lam1 = abcutil.optimize_box_cox(X[:, 0], ctx=gpu_ctx)                   # the reference's signature: one column, one lambda
    assert isinstance(lam1, float) and lam1 == m["lam"][0]
    auto = abcutil.box_cox_metrics(X - X.min(axis=0), shift="auto", ctx=gpu_ctx)     # a zero in every column: shifted by 1
    assert np.all(auto["shift"] == 1.0) and not auto["status"].any() and auto["targets"] is None
