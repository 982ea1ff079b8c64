"""The posterior's moments on the device -- weights.hip k_doubled_variance, mvn.hip k_dv_from_stats, k_cov_chol (work matrix in LDS
and in the arena), k_post_tail<PP> (cov_chol_regs up to 32 parameters, cov_chol_wave above) -- against the long-double reference
of tests/_moments_ref.py, within the bounds derived there: E for the covariance entries and dv, B for the factor, E2 for the
two-pass kernel.  Every case prints its worst share of its bounds; the assertion is always share <= 1.

Largest shares seen on gfx950 (one run of this file):
    k_dv_from_stats (Gram path, P <= 64)      0.151 of diag(E)
    k_doubled_variance (P > 64, or K < 2)     0.195 of E2
    k_cov_chol                                0.0463 of B (P = 1; 0.015 beyond), 0.024 of E (strict upper triangle)
    k_post_tail<PP>                           0.0105 of B, 0.0369 of E, 0.0436 of diag(E) (dv); the same from both call sites
A constant column's dv is exactly 0.0 from both kernels.  Before k_doubled_variance centred on the first row it was not: one
run of the parent's kernel on gfx950 through abc_calculate_doubled_variance, column 7 of a (K, P) set the constant, P in {65, 130},
the K and constants of test_doubled_variance below (72 cases), returned, alike at both widths,
    c = 0.1:  5.78e-34 at K = 3;   c = 1/3:  6.23e-33 at K = 100, 6.16e-33 at K = 4097;
    c = 7.3:  6.31e-30 at K = 4097;   c = 1e-3:  9.44e-38 at K = 300, 9.41e-38 at K = 4097;   0.0 in the other 60.
gen.L and gen.dv are bit-identical to the stand-alone entries on gen.theta at every width and both call sites.

Which call site of k_post_tail a generation takes (api.hip generation_core: defer_moments = Nnext && P <= 64 && K >= 2;
moments_side_planned = defer_moments && weights from a previous set && device noise; the side stream always exists there, and
the alias mode does not enter): Kp > 0 with a previous set -> abc_moments_on_side; Kp == 0 (uniform weights) -> the deferred
moments in abc_prep_hook (so does a weighted generation under the reference noise stream, whose proposals are host code).
test_the_two_call_sites_are_the_ones_named holds the two configurations to different sites by the stage timer only the hook sets."""
import numpy as np
import pytest

import _moments_ref as MR
import _philox_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOT_SPD = -3


def _prep(ctx):
    import torch
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def _dv_dev(ctx, th):
    import torch
    from abcsmc_amd import device, _lib
    K, P = th.shape
    t = device.colmajor(th, DEV)
    dv = torch.full((P,), np.nan, dtype=torch.float64, device=DEV)
    _prep(ctx)
    ctx.check(_lib.lib().abc_doubled_variance_dev(ctx.handle, t.data_ptr(), K, P, dv.data_ptr()))
    torch.cuda.synchronize()
    return dv.cpu().numpy()


def _mvn_dev(ctx, th):
    """abc_setup_mvn_sampler_dev: the P x P result (row, column) in GSL's layout"""
    import torch
    from abcsmc_amd import device, _lib
    t = th if hasattr(th, "data_ptr") else device.colmajor(th, DEV)      # (a holder is (P, K): column-major)
    P, K = t.shape
    L = torch.full((P, P), np.nan, dtype=torch.float64, device=DEV)
    _prep(ctx)
    ctx.check(_lib.lib().abc_setup_mvn_sampler_dev(ctx.handle, t.data_ptr(), K, P, L.data_ptr()))
    torch.cuda.synchronize()
    return device.to_numpy(L)


def _err(dev, ref_ld):
    return np.abs(np.asarray(dev).astype(MR.LD) - ref_ld).astype(np.float64)


# ---- (a) doubled variance, both kernels --------------------------------------------------------------------------------------
DV_KS = [2, 3, 100, 255, 256, 257, 300, 1000, 4097]


@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("P", [1, 16, 64, 65, 130])
def test_doubled_variance(gpu_ctx, P, kind):
    """host and device entry against the reference within diag(E) (Gram path, P <= 64) or E2 (k_doubled_variance, P > 64); one
    column a constant -- each of MR.CONSTANTS in turn at every K -- whose dv must be exactly 0.0; one row gives exactly 0.0
    everywhere (k_doubled_variance, K < 2)"""
    from abcsmc_amd import abcutil
    worst = 0.0
    cc = P // 2
    for n, K in enumerate(DV_KS):
        base = MR.data(kind, K, P, 1000 * P + K)
        for j in range(len(MR.CONSTANTS)):
            c = MR.CONSTANTS[(n + P + j) % len(MR.CONSTANTS)]
            th = base.copy()
            th[:, cc] = c
            host = abcutil.calculate_doubled_variance(th, ctx=gpu_ctx)
            devv = _dv_dev(gpu_ctx, th)
            # (exactly 0.0 is asserted on the values themselves: the bound of that column is ~0, not used)
            assert host[cc] == 0.0 and devv[cc] == 0.0, (K, P, c, host[cc], devv[cc])
            assert not np.signbit(host[cc]) and not np.signbit(devv[cc])
            if j:
                continue                    # (the other columns are the same in every turn: their values are checked once;
                                            #  a single column is checked once as the constant and once as it came)
            for t, h, d in ([(th, host, devv)] if P > 1 else
                            [(th, host, devv), (base, abcutil.calculate_doubled_variance(base, ctx=gpu_ctx), _dv_dev(gpu_ctx, base))]):
                ref = MR.dv_ld(t)
                bound = MR.dv_bound_gram(t) if P <= 64 else MR.dv_bound_two_pass(t)
                s = max(MR.share(_err(h, ref), bound), MR.share(_err(d, ref), bound))
                worst = max(worst, s)
                assert s <= 1.0, (K, P, kind, s)
    th1 = MR.data(kind, 1, P, 77 + P)
    assert np.all(abcutil.calculate_doubled_variance(th1, ctx=gpu_ctx) == 0.0) and np.all(_dv_dev(gpu_ctx, th1) == 0.0)
    print("dv %s P=%d %s: worst share of %s %.3g" % ("gram" if P <= 64 else "two-pass", P, kind, "diag(E)" if P <= 64 else "E2", worst))


# ---- (b) the stand-alone factor ----------------------------------------------------------------------------------------------
def _factor_case(ctx, th, tag):
    from abcsmc_amd import abcutil
    host = abcutil.setup_mvn_sampler(th, ctx=ctx)
    devL = _mvn_dev(ctx, th)
    assert np.array_equal(host, devL), tag
    sB, sE, E, B, ref = MR.check_factor(devL, th)
    assert sB <= 1.0 and sE <= 1.0, (tag, sB, sE)
    return sB, sE


@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("P", [1, 2, 16, 63, 64, 65, 128, 138, 139, 200])
def test_cov_chol(gpu_ctx, P, kind):
    """k_cov_chol, work matrix in LDS up to 138 parameters and in the arena from 139: lower triangle and diagonal within B, the
    strict upper triangle within E of the covariance, host and device entry bit-identical"""
    wB = wE = 0.0
    for K in ([2, 300] if P == 1 else [P + 40, P + 40 + 517]):
        sB, sE = _factor_case(gpu_ctx, MR.data(kind, K, P, 31 * P + K), (P, K, kind))
        wB, wE = max(wB, sB), max(wE, sE)
    print("cov_chol P=%d %s: worst share of B %.3g, of E %.3g" % (P, kind, wB, wE))


@pytest.mark.parametrize("P", [2, 70, 139])
def test_cov_chol_not_positive_definite(gpu_ctx, P):
    """Two equal columns.  The doubled diagonal makes C + diag(C) positive definite whenever every column varies, so equal
    columns that VARY factor like any others (checked within B); equal columns that are CONSTANT leave a zero pivot: -3 from both
    entries -- LDS side (2, 70: a pivot beyond the first 64 rows), arena side (139) --, and the next call on the same context is
    right again"""
    from abcsmc_amd import abcutil, _lib
    K = P + 40
    th = MR.data("benign", K, P, 500 + P)
    th[:, P - 1] = th[:, P - 2]
    sB, sE = _factor_case(gpu_ctx, th, ("equal varying columns", P))
    bad = th.copy()
    bad[:, P - 2:] = 1.0 / 3.0
    for call in (lambda: abcutil.setup_mvn_sampler(bad, ctx=gpu_ctx), lambda: _mvn_dev(gpu_ctx, bad)):
        with pytest.raises(_lib.AbcError) as e:
            call()
        assert e.value.code == NOT_SPD
        sB2, sE2 = _factor_case(gpu_ctx, MR.data("far", K, P, 600 + P), ("after not-SPD", P))
    print("not-SPD P=%d: -3 from both entries; equal varying columns share of B %.3g, E %.3g; after: %.3g, %.3g" % (P, sB, sE, sB2, sE2))


# ---- (c) the fused tail through device.Generation -----------------------------------------------------------------------------
def _workload(P, seed, far, const_col=None):
    """(X, Y, obs, spec, wl): synthetic.Workload rows, the parameter columns offset by 1e6 sd (far), one of them constant"""
    from abcsmc_amd import synthetic
    wl = synthetic.Workload(8, P, seed)
    off = (1e6 * wl.sd_y * np.where(np.arange(P) % 2, -1.0, 1.0)) if far else np.zeros(P)
    X, Y = wl.rows(0, 2000)
    Y = np.asfortranarray(Y + off)
    mu = wl.mu_y + off
    if const_col is not None:
        Y[:, const_col] = mu[const_col]
    spec = [(R.UNIF_REAL, mu[j] - 6 * wl.sd_y[j], mu[j] + 6 * wl.sd_y[j]) if j % 2 == 0 else (R.GAUSS, mu[j], 3 * wl.sd_y[j])
            for j in range(P)]
    return X, Y, wl.observed(), spec, wl, off


def _generation(ctx, P, K, site, far, seed, Nn=2001, const_col=None):
    """one multivariate generation; site "side": Kp = 300 with a previous set (abc_moments_on_side), "hook": Kp = 0 (abc_prep_hook)"""
    import torch
    from abcsmc_amd import abcutil, device, _lib
    X, Y, obs, spec, wl, off = _workload(P, seed, far, const_col)
    Kp = 300 if site == "side" else 0
    gen = device.Generation(X.shape[0], 8, P, K, Kp, Nn, 0.5, 4, multivariate=True, device=DEV, ctx=ctx)
    r = abcutil.rng(4242 + P + K)
    key = R.philox_key(r.s1, r.s2, r.s3)          # launch_perturb is keyed by the rng state the call was entered with
    prev = ()
    if Kp:
        tp, wp, dvp = wl.previous_set(Kp)
        prev = tuple(device.colmajor(a, DEV) for a in (tp + off, wp, dvp))
    gen.run(device.colmajor(X, DEV), device.colmajor(Y, DEV), device.colmajor(obs, DEV),
            device.priors_to_device(_lib.make_priors(spec), DEV), r, *prev)
    torch.cuda.synchronize()
    return gen, key, spec


def _check_generation(ctx, gen, key, spec, tag):
    """gen.L, gen.dv within the bounds and bit-identical to the stand-alone entries on gen.theta; gen.next against the model"""
    from abcsmc_amd import device
    th = device.to_numpy(gen.theta)
    Lg = device.to_numpy(gen.L)
    dv = gen.dv.cpu().numpy()
    sB, sE, E, B, ref = MR.check_factor(Lg, th)
    sD = MR.share(_err(dv, np.diag(ref["cov"])), np.diag(E))
    assert sB <= 1.0 and sE <= 1.0 and sD <= 1.0, (tag, sB, sE, sD)
    assert np.array_equal(Lg, _mvn_dev(ctx, gen.theta)), tag
    assert np.array_equal(dv, _dv_dev(ctx, th)), tag
    Nn = gen.cfg.Nnext
    par = gen.parent.cpu().numpy().astype(np.int64)
    x = device.to_numpy(gen.next)
    pr = R.proposals_ref(key, th, par, spec, np.tril(Lg), True, 0, Nn)
    keep = ~pr["ambiguous"]
    err = np.abs(x - pr["x"])
    bad = keep[:, None] & ~(err <= pr["tol"])
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[0])
    assert pr["ambiguous"].mean() < 0.001, (tag, int(pr["ambiguous"].sum()))
    return sB, sE, sD


@pytest.mark.parametrize("site", ["side", "hook"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64])
def test_post_tail(gpu_ctx, P, site):
    """k_post_tail<PP> at both edges of every PP, K across a 64-row tile of the row-major copy and across the 256-row pilot,
    the selected theta near zero and 1e6 sd from it, from both call sites"""
    wB = wE = wD = 0.0
    for K in ([65, 257] if P <= 32 else [130, 257]):
        for far in (False, True):
            tag = "P=%d K=%d %s %s" % (P, K, site, "far" if far else "near")
            gen, key, spec = _generation(gpu_ctx, P, K, site, far, 12345 + P)
            sB, sE, sD = _check_generation(gpu_ctx, gen, key, spec, tag)
            wB, wE, wD = max(wB, sB), max(wE, sE), max(wD, sD)
    print("post_tail P=%d %s: worst share of B %.3g, of E %.3g, of diag(E) (dv) %.3g" % (P, site, wB, wE, wD))


def test_the_two_call_sites_are_the_ones_named(gpu_ctx):
    """What tells the sites apart from outside: abc_prep_hook brackets its deferred moments with the gather_dv stage timer,
    abc_moments_on_side runs on the side stream under no timer; the gather itself is bracketed in both.  The same ranking (the
    previous set does not enter it) therefore counts one gather_dv bracket more through the hook -- if the conditions in
    generation_core change so that "side" and "hook" above take the same site, this fails.  Timing changes no result"""
    count = {}
    for site in ("side", "hook"):
        gpu_ctx.timing_enable(True)
        try:
            gpu_ctx.timing_read(reset=True)
            gen, key, spec = _generation(gpu_ctx, 8, 65, site, False, 12345 + 8)
            count[site] = gpu_ctx.timing_read(reset=True)["gather_dv"][2]
        finally:
            gpu_ctx.timing_enable(False)
        _check_generation(gpu_ctx, gen, key, spec, "timed P=8 %s" % site)
    print("gather_dv brackets: %s" % count)
    assert count["hook"] == count["side"] + 1, count


@pytest.mark.parametrize("site", ["side", "hook"])
@pytest.mark.parametrize("P", [3, 33])
def test_generation_not_positive_definite(gpu_ctx, P, site):
    """a constant parameter column: the zero pivot in cov_chol_regs (3) and in cov_chol_wave inside k_post_tail<64> (33) reaches
    the host through the pinned status word, and the generation fails with -3; the next generation on the same context is right"""
    from abcsmc_amd import _lib
    with pytest.raises(_lib.AbcError) as e:
        _generation(gpu_ctx, P, 130, site, False, 777 + P, const_col=1)
    assert e.value.code == NOT_SPD
    gen, key, spec = _generation(gpu_ctx, P, 130, site, False, 778 + P)
    shares = _check_generation(gpu_ctx, gen, key, spec, "after not-SPD P=%d %s" % (P, site))
    print("generation not-SPD P=%d %s: -3, then shares %s" % (P, site, shares))
