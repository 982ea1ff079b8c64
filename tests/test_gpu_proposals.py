"""The device-noise proposals (resample.hip: k_perturb<PP, MV>, k_perturb_stream<64, false>, k_perturb_gen<MV>; mvn.hip:
k_post_tail<PP>) against the host model of their stream (tests/_philox_ref.py), value by value, at every kernel width.

The model reproduces the Philox words exactly and the deviates up to the f32 transcendental hardware: a proposal must lie within
sum_b |L_ab| zbound_b (+ roundings) of the model's, integer coordinates must be equal.  A wrong counter word, key, column, row
group, padded-factor layout or slice offset moves a proposal by O(1) in units of its noise.

The factor and the doubled variance k_post_tail computes are held to the long-double reference and the derived bounds of
tests/_moments_ref.py here at one shape per width (test_generation_factor_and_proposals); tests/test_gpu_moments.py pins them at
every width, both call sites and the stand-alone kernels.

zbound (tests/_philox_ref.py: ZB_MULT x the first-order error of one unit in each hardware step) was set from one measured run of
test_hardware_deviates_against_the_model on gfx950: over 1.6e6 deviates the largest |z_dev - z_ref| was 6.1e-4, 0.999 units of
the model (ZB_MULT = 16: 16x headroom).  That worst case is one ulp of v_log_f32 near 32 (u close to 1, a small radius); for
|z| > 0.1 the largest relative error was 1.3e-4, for typical deviates it is ~1e-6 (declared deviations)."""
import ctypes as C

import numpy as np
import pytest

import _moments_ref as MR
import _philox_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100, 130]
NEVER = (R.UNIF_REAL, -1e300, 1e300)


def _key(r):
    return R.philox_key(r.s1, r.s2, r.s3)


def _perturb(ctx, rng, theta, spec, parent, i0, multivariate, L_or_dv, seeds=False, seed_off=0):
    """abc_perturb_dev on rows i0 .. i0 + n - 1 (n = len(parent)): (n, P) proposals [, seeds]"""
    import torch
    from abcsmc_amd import device, _lib
    dev = "cuda:0"
    K, P = theta.shape
    n = len(parent)
    th = device.colmajor(theta, dev)
    pr = device.priors_to_device(_lib.make_priors(spec), dev)
    par = torch.from_numpy(np.asarray(parent, dtype=np.int64)).to(dev)
    lv = device.colmajor(np.asarray(L_or_dv, dtype=np.float64), dev)
    out = torch.empty((P, n), dtype=torch.float64, device=dev)
    sd = torch.empty(n, dtype=torch.int64, device=dev) if seeds else None
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(_lib.lib().abc_perturb_dev(ctx.handle, C.byref(rng), th.data_ptr(), K, P, pr.data_ptr(), par.data_ptr(), int(i0),
                                         n, int(multivariate), lv.data_ptr(), out.data_ptr(), sd.data_ptr() if seeds else None,
                                         int(seed_off)))
    torch.cuda.synchronize()
    x = device.to_numpy(out)
    return (x, sd.cpu().numpy().astype(np.uint64)) if seeds else x


def _factor(g, P, scale):
    """a well-conditioned lower factor of a correlated covariance with per-coordinate scales"""
    A = g.normal(size=(P, P)) / np.sqrt(P)
    C_ = (A @ A.T + np.eye(P)) * np.outer(scale, scale)
    return np.linalg.cholesky(C_)


def _check(x, ref, tag, max_ambiguous=0.001):
    """every non-ambiguous row within the model's bound (integer coordinates exact); the ambiguous share below max_ambiguous"""
    amb = ref["ambiguous"]
    keep = ~amb
    err = np.abs(x - ref["x"])
    bad = keep[:, None] & ~(err <= ref["tol"])
    if bad.any():
        i, p = np.argwhere(bad)[0]
        raise AssertionError("%s: %d coordinates outside the bound, first row %d col %d: dev %r ref %r tol %g (attempt %d)"
                             % (tag, bad.sum(), i, p, x[i, p], ref["x"][i, p], ref["tol"][i, p], ref["attempt"][i]))
    print("%s: %d rows, %d ambiguous, worst |dev - ref| / tol %.3g" % (tag, len(x), amb.sum(),
                                                                       np.max(np.where(ref["tol"] > 0, err / np.maximum(ref["tol"], 1e-300), 0.0)[keep])))
    assert amb.mean() < max_ambiguous, (tag, amb.sum())


def test_hardware_deviates_against_the_model(gpu_ctx):
    """L = I, zero parents, priors that never reject: the proposals ARE the device deviates (fma(1, z, 0) and the zero
    products are exact), one Philox block per four columns.  Measures the hardware error in units of the model and holds it to
    zbound (ZB_MULT units)"""
    from abcsmc_amd import abcutil
    worst_units, worst_abs, worst_rel, worst_rel1 = 0.0, 0.0, 0.0, 0.0
    for P, n, i0 in [(8, 40001, 5), (64, 20001, (7 << 32) + 3)]:
        r = abcutil.rng(1000 + P)
        th = np.zeros((3, P))
        par = np.arange(n) % 3
        x = _perturb(gpu_ctx, r, th, [NEVER] * P, par, i0, True, np.eye(P))
        gi = np.uint64(i0) + np.arange(n, dtype=np.uint64)
        zs, us = [], []
        for qd in range(P // 4):
            z, zb = R.normal4_ref(R.philox4x32_10(R._counters(gi, 0, qd), *_key(r)))
            zs.append(z)
            us.append(zb / R.ZB_MULT)
        z, u = np.concatenate(zs).T, np.concatenate(us).T
        d = np.abs(x - z)
        worst_units = max(worst_units, float(np.max(d / u)))
        worst_abs = max(worst_abs, float(d.max()))
        worst_rel = max(worst_rel, float(np.max(d[np.abs(z) > 0.1] / np.abs(z[np.abs(z) > 0.1]))))
        worst_rel1 = max(worst_rel1, float(np.max(d[np.abs(z) > 1.0] / np.abs(z[np.abs(z) > 1.0]))))
    print("hardware deviates: worst |z_dev - z_ref| %.3g, %.3g relative (|z| > 0.1), %.3g (|z| > 1), %.3g units of the model "
          "(bound %g units)" % (worst_abs, worst_rel, worst_rel1, worst_units, R.ZB_MULT))
    assert worst_units * 8.0 <= R.ZB_MULT
    assert worst_abs < 1e-3 and worst_rel1 < 1e-5


def _never_case(P, seed):
    g = np.random.default_rng(seed)
    K = 37
    scale = 10.0 ** g.uniform(-2, 2, P)
    th = g.normal(size=(K, P)) * scale * 3.0
    spec = [NEVER if p % 2 == 0 else (R.GAUSS, 0.0, 1e9) for p in range(P)]
    return g, K, scale, th, spec


@pytest.mark.parametrize("P", WIDTHS)
def test_proposals_without_rejection_match_the_model(gpu_ctx, P):
    """(a) both noise kinds, given parents, i0 > 0 (its high word too), odd n: every coordinate within the model's bound"""
    from abcsmc_amd import abcutil
    g, K, scale, th, spec = _never_case(P, 100 + P)
    n = 20001 if P <= 64 else 8001
    par = g.integers(0, K, n)
    i0 = (P << 32) + 1001
    L = _factor(g, P, scale)
    r = abcutil.rng(500 + P)
    x = _perturb(gpu_ctx, r, th, spec, par, i0, True, L)
    ref = R.proposals_ref(_key(r), th, par, spec, L, True, i0, n)
    assert np.all(ref["attempt"] == 0)
    _check(x, ref, "mv P=%d" % P, max_ambiguous=1e-300)
    dv = 2.0 * scale ** 2
    x = _perturb(gpu_ctx, r, th, spec, par, i0, False, dv)
    ref = R.proposals_ref(_key(r), th, par, spec, dv, False, i0, n)
    _check(x, ref, "indep P=%d" % P, max_ambiguous=1e-300)


def _rejecting_case(P, seed):
    """narrow uniform, integer, far-edge Gaussian (parents ~37.9 sd from the mean: the exact support test runs, rarely rejects),
    huge-sigma Gaussian (always the exact test) and never-rejecting coordinates; proposal sd per coordinate in `sd`"""
    g = np.random.default_rng(seed)
    K = 53
    cols, spec, sd = [], [], []
    for p in range(P):
        k = p % 8
        if k in (0, 4):
            cols.append(g.uniform(0.03, 0.97, K)); spec.append((R.UNIF_REAL, 0.0, 1.0)); sd.append(0.02)
        elif k == 1:
            cols.append(np.round(g.uniform(2, 98, K))); spec.append((R.UNIF_INT, 0, 100)); sd.append(0.2)
        elif k == 2:
            s = 10.0 ** g.uniform(-1, 1)
            cols.append(g.uniform(37.85, 37.95, K) * s); spec.append((R.GAUSS, 0.0, s)); sd.append(0.1 * s)
        elif k == 5:
            cols.append(g.normal(0, 1, K)); spec.append((R.GAUSS, 1.0, 2e10)); sd.append(1.0)
        else:
            cols.append(g.normal(0, 3, K)); spec.append(NEVER); sd.append(1.0)
    return g, K, np.column_stack(cols), spec, np.array(sd)


@pytest.mark.parametrize("P", WIDTHS)
def test_proposals_with_rejection_match_the_model(gpu_ctx, P):
    """(b) rejecting priors: non-ambiguous rows within the bound, integer coordinates exact, the ambiguous share < 0.1 %, the
    give-up count equal to the model's"""
    from abcsmc_amd import abcutil
    g, K, th, spec, sd = _rejecting_case(P, 300 + P)
    n = 20001 if P <= 64 else 8001
    par = g.integers(0, K, n)
    i0 = 77 + 3 * P
    r = abcutil.rng(700 + P)
    L = _factor(g, P, sd)
    gpu_ctx.perturb_giveups(reset=True)
    x = _perturb(gpu_ctx, r, th, spec, par, i0, True, L)
    ref = R.proposals_ref(_key(r), th, par, spec, L, True, i0, n)
    _check(x, ref, "mv P=%d (%d rejected first candidates)" % (P, np.count_nonzero(ref["attempt"] != 0)))
    assert gpu_ctx.perturb_giveups(reset=True) == ref["giveups"]
    dv = sd ** 2
    x = _perturb(gpu_ctx, r, th, spec, par, i0, False, dv)
    ref = R.proposals_ref(_key(r), th, par, spec, dv, False, i0, n)
    _check(x, ref, "indep P=%d" % P)
    assert gpu_ctx.perturb_giveups(reset=True) == ref["giveups"]


@pytest.mark.parametrize("P", [1, 4, 33, 65])
def test_independent_give_ups_match_the_model(gpu_ctx, P):
    """a coordinate that accepts ~0.7 % of its candidates: some rows run out of their 1000 tries and take the prior mean --
    which rows, and how many, as the model says"""
    from abcsmc_amd import abcutil
    g = np.random.default_rng(900 + P)
    K, n = 11, 3001
    th = np.column_stack([np.full(K, 0.0)] + [g.normal(size=K) for _ in range(P - 1)])
    spec = [(R.UNIF_REAL, 2.45, 2.5)] + [NEVER] * (P - 1)
    dv = np.ones(P)
    par = g.integers(0, K, n)
    r = abcutil.rng(31 + P)
    gpu_ctx.perturb_giveups(reset=True)
    x = _perturb(gpu_ctx, r, th, spec, par, 12, False, dv)
    ref = R.proposals_ref(_key(r), th, par, spec, dv, False, 12, n)
    assert 0 < ref["giveups"] < n
    # (up to 1000 candidates per row: ~0.1 % of the rows meet an edge within its bound somewhere on the way)
    _check(x, ref, "indep give-ups P=%d (%d)" % (P, ref["giveups"]), max_ambiguous=0.01)
    amb = ref["ambiguous"]
    assert abs(gpu_ctx.perturb_giveups(reset=True) - ref["giveups"]) <= amb.sum()
    assert np.array_equal((x[:, 0] == 2.475)[~amb], (ref["x"][:, 0] == 2.475)[~amb])


@pytest.mark.parametrize("P", [2, 3, 16, 32, 48, 100])
@pytest.mark.parametrize("multivariate", [True, False])
def test_row_slices_equal_one_call(gpu_ctx, oracle, P, multivariate):
    """(c) [0, a), [a, b), [b, n) called separately equal one [0, n) call bit for bit; the seeds are the taus2 outputs at
    seed_stream_offset + i0 + i"""
    from abcsmc_amd import abcutil
    g, K, th, spec, sd = _rejecting_case(P, 50 + P)
    n, a, b, off = 5001, 1234, 3000, 1500
    par = g.integers(0, K, n)
    L = _factor(g, P, sd) if multivariate else sd ** 2
    whole, seeds = _perturb(gpu_ctx, abcutil.rng(9), th, spec, par, 0, multivariate, L, seeds=True, seed_off=off)
    for lo, hi in [(0, a), (a, b), (b, n)]:
        part, s = _perturb(gpu_ctx, abcutil.rng(9), th, spec, par[lo:hi], lo, multivariate, L, seeds=True, seed_off=off)
        assert np.all(part == whole[lo:hi]), (lo, hi)
        assert np.array_equal(s, seeds[lo:hi])
    o = oracle.rng(9)
    for _ in range(off):
        oracle.rng_get(o)
    assert np.array_equal(seeds, np.array([oracle.rng_get(o) for _ in range(n)], dtype=np.uint64))


CHAIN = [2, 3, 8, 20, 40, 100]


@pytest.mark.parametrize("multivariate", [True, False])
def test_column_prefix_of_a_wider_call(gpu_ctx, multivariate):
    """(c) columns 0 .. p - 1 of a P-wide call equal a p-wide call with those columns, bit for bit, across kernels of every width
    (k_perturb<2..64>, k_perturb_stream, k_perturb_gen).  Multivariate: the factor is extended block-lower by rows whose priors
    never reject, so the acceptance does not change; the products the wider kernels skip are exact zeros and the fma order is
    the same in every kernel"""
    from abcsmc_amd import abcutil
    g, K, th, spec, sd = _rejecting_case(CHAIN[0], 11)
    L = _factor(g, CHAIN[0], sd) if multivariate else sd ** 2
    for P in CHAIN[1:]:
        extra = P - th.shape[1]
        th = np.column_stack([th, g.normal(size=(K, extra))])
        spec = spec + [NEVER] * extra
        if multivariate:
            Lw = np.zeros((P, P))
            Lw[:L.shape[0], :L.shape[0]] = L
            Lw[L.shape[0]:, :] = np.tril(g.normal(size=(extra, P)) * 0.3, L.shape[0])
            Lw[np.arange(L.shape[0], P), np.arange(L.shape[0], P)] = 1.0
            L = Lw
        else:
            L = np.concatenate([L, g.uniform(0.5, 2.0, extra)])
    n = 4097
    par = g.integers(0, K, n)
    prev = None
    for P in reversed(CHAIN):
        Lp = L[:P, :P] if multivariate else L[:P]
        x = _perturb(gpu_ctx, abcutil.rng(21), th[:, :P], spec[:P], par, 999, multivariate, Lp)
        if prev is not None:
            assert np.all(prev[:, :P] == x), (P, np.argwhere(prev[:, :P] != x)[:3])
        prev = x


# ---- the fused generation: k_post_tail's factor, padded factor and parent table ---------------------------------------------
@pytest.mark.parametrize("P", [2, 3, 5, 8, 9, 17, 32, 33, 64])
def test_generation_factor_and_proposals(gpu_ctx, P):
    """(d) a small weighted multivariate generation: gen.L and gen.dv against a long-double reference from gen.theta (the doubled
    n - 1 covariance, then its Cholesky factor), and gen.next against the model on the generation's own theta, parents, factor
    and entry rng state -- what k_post_tail hands k_perturb (its padded factor and row-major parent table) at every width.

    The statistics of a set this small come from the fp64 Gram kernels (the byte-limb kernel of tests/_gram_model.py needs
    >= 400000 rows): the covariance is bounded by the fp64 rounding of sums of K products, the factor by that error times
    the condition number (E and B of tests/_moments_ref.py; B stays below 1e-10 of the largest factor entry here, where the
    oracle comparisons ask for rtol 1e-7)"""
    import torch
    from abcsmc_amd import abcutil, device, synthetic, _lib
    N, M, K, Kp, Nn, A = 3000, 8, 600, 300, 4001, 4
    wl = synthetic.Workload(M, P, 12345)
    X, Y = wl.rows(0, N)
    spec = wl.prior_spec()
    prev = wl.previous_set(Kp)
    dev = "cuda:0"
    gen = device.Generation(N, M, P, K, Kp, Nn, 0.5, A, multivariate=True, device=dev, ctx=gpu_ctx)
    r = abcutil.rng(4242 + P)
    key = _key(r)                       # abc_generation_dev: launch_perturb is keyed by the rng state the call was entered with
    gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(wl.observed(), dev),
            device.priors_to_device(_lib.make_priors(spec), dev), r, *(device.colmajor(a, dev) for a in prev))
    torch.cuda.synchronize()
    th = device.to_numpy(gen.theta)
    Lg = device.to_numpy(gen.L)
    L = np.tril(Lg)
    dv = gen.dv.cpu().numpy()
    # long-double reference and derived bounds (tests/_moments_ref.py): covariance with n - 1, its diagonal doubled
    # (AbcUtil.cpp:475-479), then the factor; the strict upper triangle keeps the covariance entries
    sB, sE, E, B, mref = MR.check_factor(Lg, th)
    Lr = mref["L"]
    err = np.abs(L - Lr)
    dv_ref = mref["dv"]
    print("P=%d: |L - L_ref| %.3g, worst share of B %.3g, of E (strict upper triangle) %.3g, bound / max|L| %.3g, |dv - dv_ref| / dv %.3g" % (
        P, err.max(), sB, sE, B.max() / np.abs(Lr).max(), np.max(np.abs(dv - dv_ref) / dv)))
    assert sB <= 1.0 and sE <= 1.0 and B.max() < 1e-10 * np.abs(Lr).max()
    assert np.all(np.abs(dv.astype(MR.LD) - np.diag(mref["cov"])).astype(np.float64) <= np.diag(E))
    par = gen.parent.cpu().numpy().astype(np.int64)
    x = device.to_numpy(gen.next)
    ref = R.proposals_ref(key, th, par, spec, L, True, 0, Nn)
    _check(x, ref, "generation P=%d" % P)
