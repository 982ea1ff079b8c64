"""CPU checks of tests/_weights_ref.py, the long-double reference of the weight stage's tests, against the oracle
(oracle/abc_oracle.cpp: orc_weights_importance, orc_weights_epanechnikov) wherever the oracle's plain products are normal
numbers: 1e-12 relative on the normalised weights (measured: 6.6e-15 at most), all three prior kinds, a converged parameter
under both policies, previous weights of exactly 0, the Epanechnikov form -- and cases whose pair terms all lie below 1e-300,
where the oracle underflows and the reference must not."""
import numpy as np
import pytest

import _weights_ref as R

GAUSS, UNIF_INT, UNIF_REAL = R.PRIOR_GAUSS, R.PRIOR_UNIF_INT, R.PRIOR_UNIF_REAL
TOL = 1e-12


def _case(P, K, Kp, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    sd = 10.0 ** rng.uniform(-2, 3, P)
    mu = sd * rng.uniform(-5, 5, P)
    tp = mu + 0.5 * spread * sd * rng.normal(size=(Kp, P))
    th = mu + 0.4 * spread * sd * rng.normal(size=(K, P))
    wp = rng.random(Kp)
    wp /= np.linalg.norm(wp)
    dv = 2.0 * tp.var(axis=0, ddof=1)
    spec = [(UNIF_REAL, mu[p] - 6 * sd[p], mu[p] + 6 * sd[p]) if p % 2 == 0 else (GAUSS, mu[p], 3 * sd[p]) for p in range(P)]
    return spec, th, tp, wp, dv, sd


def _relerr(w, ref):
    ok = ref != 0
    assert np.array_equal(w == 0, ref == 0)
    return float(np.max(np.abs(w[ok] - ref[ok]) / np.abs(ref[ok])))


@pytest.mark.parametrize("P,K,Kp", [(20, 300, 1200), (61, 200, 700), (7, 400, 600)])
def test_reference_matches_the_oracle(oracle, P, K, Kp):
    """the shapes of the GPU tests, with previous weights of 0 and one far row on each side"""
    spec, th, tp, wp, dv, sd = _case(P, K, Kp, 100 + P, spread=0.6 if P > 40 else 1.0)
    wp[::53] = 0.0
    th[11, 3] += 9.0 * np.sqrt(dv[3])
    tp[17, P - 1] -= 8.0 * np.sqrt(dv[P - 1])
    ref = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv)
    assert np.all(np.isfinite(ref)) and np.all(ref > 0)
    w = R.normalised(spec, th, tp, wp, dv)
    err = _relerr(w, ref)
    print("P = %d K = %d K' = %d: reference against the oracle %.2e" % (P, K, Kp, err))
    assert err < TOL
    assert np.linalg.norm(w) == pytest.approx(1.0, rel=1e-14)
    # raw(): the same weights before the normalisation -- proportional, and equal to the oracle's own ratio for one row
    raw = R.raw(spec, th, tp, wp, dv)
    assert raw.dtype == np.longdouble and np.max(np.abs((raw / raw[0]).astype(float) * ref[0] / ref - 1.0)) < TOL


def test_all_three_prior_kinds_and_their_supports(oracle):
    spec, th, tp, wp, dv, sd = _case(6, 250, 300, 9)
    spec[1] = (UNIF_INT, 1, 10)
    th[:, 1] = np.random.default_rng(1).integers(-1, 13, 250)            # some outside [1, 10] ...
    th[7, 1] = 4.5                                                       # ... and one that is no integer
    tp[:, 1] = np.random.default_rng(2).integers(1, 11, 300)
    dv[1] = 2.0 * tp[:, 1].var(ddof=1)
    spec[2] = (UNIF_REAL, float(np.median(th[:, 2])), float(th[:, 2].max() + 1))     # half outside the support
    spec[3] = (GAUSS, float(th[:, 3].mean()), -2.0 * sd[3])              # (the density takes |sigma|)
    th[9, 2] = spec[2][1]                                                # on the closed ends of the support
    th[10, 2] = spec[2][2]
    th[[9, 10], 1] = 5.0
    ref = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv)
    w = R.normalised(spec, th, tp, wp, dv)
    assert 60 < (ref == 0).sum() < 200 and ref[7] == 0 and ref[9] > 0 and ref[10] > 0
    assert _relerr(w, ref) < TOL
    num = R.prior_product(spec, th)
    for i in (0, 7, 9, 10, 100):
        o = np.prod([oracle.prior_likelihood(oracle.make_priors(spec)[p], th[i, p]) for p in range(6)])
        assert float(num[i]) == pytest.approx(o, rel=1e-13)


def test_converged_parameter_under_both_policies(oracle):
    spec, th, tp, wp, dv, sd = _case(5, 120, 150, 21)
    spec[1] = (UNIF_INT, 1, 10)
    th[:, 1] = 7.0
    tp[:, 1] = 7.0
    dv[1] = 0.0
    pri = oracle.make_priors(spec)
    # every value equal: factor 1 under both policies (AbcUtil.cpp:573)
    for policy in (0, 1):
        ref = oracle.weights_importance(pri, th, tp, wp, dv, policy)
        assert np.all(ref > 0) and _relerr(R.normalised(spec, th, tp, wp, dv, policy), ref) < TOL
    # some previous rows differ: policy 0 drops their terms (the declared deviation) ...
    tp[::7, 1] = 8.0
    th[::5, 1] = 8.0                                                     # (these new rows keep only the terms of the rows that moved)
    ref = oracle.weights_importance(pri, th, tp, wp, dv, 0)
    w = R.normalised(spec, th, tp, wp, dv, 0)
    assert np.all(ref > 0) and _relerr(w, ref) < TOL
    keep = tp[:, 1] == 7.0
    i7 = th[:, 1] == 7.0
    part = R.raw(spec, th[i7], tp[keep], wp[keep], dv)                   # the same weights from the rows that are left
    assert np.max(np.abs((part / R.raw(spec, th, tp, wp, dv)[i7]).astype(float) - 1.0)) < 1e-15
    # ... and policy 1 evaluates the reference's Gaussian of deviation 0: NaN
    ref1 = oracle.weights_importance(pri, th, tp, wp, dv, 1)
    raw1 = R.raw(spec, th, tp, wp, dv, 1)
    assert np.all(np.isnan(ref1)) and np.all(np.isnan(raw1)) and np.all(np.isnan(R.normalised(spec, th, tp, wp, dv, 1)))
    # a new row that no previous row equals: denominator 0 under policy 0, as in the oracle
    th[3, 1] = 9.0
    ref = oracle.weights_importance(pri, th, tp, wp, dv, 0)
    assert np.isinf(R.raw(spec, th, tp, wp, dv, 0)[3]) and not np.isfinite(ref).all()


def test_previous_weights_of_zero_contribute_nothing(oracle):
    spec, th, tp, wp, dv, sd = _case(9, 90, 200, 33)
    wp[::3] = 0.0
    ref = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv)
    w = R.normalised(spec, th, tp, wp, dv)
    assert _relerr(w, ref) < TOL
    keep = wp != 0.0
    assert np.array_equal(w, R.normalised(spec, th, tp[keep], wp[keep], dv))
    # every weight 0: the oracle divides by 0; so does the reference
    assert np.all(np.isinf(R.raw(spec, th, tp, 0.0 * wp, dv)) | np.isnan(R.raw(spec, th, tp, 0.0 * wp, dv)))


@pytest.mark.parametrize("P,K,Kp,conv", [(3, 300, 257, False), (16, 200, 700, True), (40, 129, 64, True)])
def test_epanechnikov_form(oracle, P, K, Kp, conv):
    spec, th, tp, wp, dv, sd = _case(P, K, Kp, 7 + P)
    if conv:
        dv[2] = 0.0                                                      # a converged parameter takes no part
    th[5] = th[5] + 40 * np.sqrt(np.where(dv > 0, dv, 1.0))              # far from everything: no support
    ref = oracle.weights_epanechnikov(oracle.make_priors(spec), th, tp, wp, dv)
    w = R.epanechnikov(spec, th, tp, wp, dv)
    assert w[5] == 0.0 and ref[5] == 0.0 and (ref > 0).sum() > K // 2
    assert _relerr(w, ref) < TOL
    raw = R.epanechnikov(spec, th, tp, wp, dv, normalise=False)
    assert raw.dtype == np.longdouble and np.array_equal(R._normalise(raw), w)


@pytest.mark.parametrize("kind", ["weights", "distance"])
def test_terms_below_1e300_keep_their_digits(oracle, kind):
    """every pair term below 1e-300: the oracle's plain products underflow (its denominators are 0 or subnormal), the reference
    gives the weights of the same set with the common factor taken out"""
    P, K, Kp = 12, 60, 150
    spec, th, tp, wp, dv, sd = _case(P, K, Kp, 55)
    th, tp, dv = 1e3 * th, 1e3 * tp, 1e6 * dv            # deviations of 10 .. 1e6: every Gaussian factor below 0.06
    spec = [(GAUSS, 0.0, 1e8)] * P
    base = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp, dv)
    assert np.all(np.isfinite(base)) and np.all(base > 0)
    assert _relerr(R.normalised(spec, th, tp, wp, dv), base) < TOL
    if kind == "weights":
        # previous weights scaled by 2^-1000 (normal numbers still): a common factor of every denominator, gone after the
        # normalisation
        wp_small = wp * 2.0 ** -1000
        assert wp_small.max() < 1e-300 and wp_small.min() > 2.3e-308
        ld = R.log_denominator(th, tp, wp_small, dv)
        assert float(ld.max()) < np.log(1e-308)                          # (every denominator below the normal numbers)
        sunk = oracle.weights_importance(oracle.make_priors(spec), th, tp, wp_small, dv)
        assert not (np.all(np.isfinite(sunk)) and _relerr(sunk, base) < 1e-6)        # the oracle: denominators of 0 or a few bits
        w = R.normalised(spec, th, tp, wp_small, dv)
        assert _relerr(w, base) < TOL
        ratio = R.raw(spec, th, tp, wp_small, dv) / R.raw(spec, th, tp, wp, dv)
        assert np.max(np.abs((ratio * np.longdouble(2.0) ** -1000).astype(float) - 1.0)) < 1e-15
    else:
        # every new row 42 deviations from every previous one in one coordinate: terms near exp(-880)
        th2 = th.copy()
        th2[:, 4] += 42.0 * np.sqrt(dv[4])
        sunk = oracle.weights_importance(oracle.make_priors(spec), th2, tp, wp, dv)
        assert not np.all(np.isfinite(sunk) & (sunk > 0))
        ld = R.log_denominator(th2, tp, wp, dv)
        assert np.all(np.isfinite(ld)) and float(ld.max()) < np.log(1e-300)
        w = R.normalised(spec, th2, tp, wp, dv)
        assert np.all(np.isfinite(w)) and np.all(w > 0)
        # the same set with that coordinate's gap removed analytically: for each pair the term is
        # exp(-((d + g)^2 - d^2) / (2 dv)) times the ungapped one, g the gap; summed directly in long double
        LD = np.longdouble
        g = LD(42.0) * np.sqrt(LD(dv[4]))
        d = (th2[:, 4].astype(LD) - g)[:, None] - tp[:, 4].astype(LD)[None, :]
        # (th2 - g is not th bit for bit: rebuild the ungapped terms from th2 - g itself)
        th0 = th.astype(LD).copy()
        th0[:, 4] = th2[:, 4].astype(LD) - g
        terms = np.zeros((K, Kp), dtype=LD)
        for p in range(P):
            dd = th0[:, p][:, None] - tp[:, p].astype(LD)[None, :]
            terms -= dd * dd / (2 * LD(dv[p]))
        terms += -((d + g) ** 2 - d ** 2) / (2 * LD(dv[4])) + np.log(wp.astype(LD))[None, :]
        direct = np.log(np.exp(terms - terms.max()).sum(axis=1)) + terms.max() - sum(np.log(2 * np.pi * LD(x)) / 2 for x in dv)
        assert np.max(np.abs((direct - ld) / ld).astype(float)) < 1e-15
