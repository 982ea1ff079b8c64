"""CPU: the log / logit parameter transforms of the local-linear adjustment (include/abcsmc_hip.h, abc_ctx_set_param_transf).  The
new entries are bound, the NumPy form of the definition (abcutil.transform_params / untransform_params) does what the header
says, the case that motivates the transforms is real for the reference regression alone, and the wrappers hand transf / bounds on
only when they are given (no GPU call)."""
import subprocess

import numpy as np
import pytest

import _loclinear_ref as R
from test_loclinear_cpu import ROOT, _header_args


def test_abi_entries_bound():
    from abcsmc_amd import _lib
    for n in ("abc_ctx_set_param_transf", "abc_param_transf_dev", "abc_param_transf", "abc_param_transf_outside"):
        assert n in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[n][1]) == len(_header_args(n)), n
    assert [f[0] for f in _lib.ParamTransf._fields_] == ["P", "kind", "lo", "hi"]
    assert (_lib.TRANSF_NONE, _lib.TRANSF_LOG, _lib.TRANSF_LOGIT) == (0, 1, 2)
    for name in ("set_param_transf", "param_transf", "param_transf_outside"):
        assert callable(getattr(_lib.Context, name))


def test_facade_declares_transforms():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "ABC::Mat2D f(const ABC::Mat2D& V) {\n"
           "  ABC::set_param_transf({ABC_TRANSF_LOG, ABC_TRANSF_NONE, ABC_TRANSF_LOGIT}, {0, 0, -1}, {0, 0, 3});\n"
           "  ABC::Mat2D t = ABC::param_transf(V, false);\n"
           "  ABC::Mat2D y = ABC::param_transf(t, true);\n"
           "  ABC::clear_param_transf();\n"
           "  return y; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


KINDS = ("log", "logit", "none")
BOUNDS = np.array([[0.0, 0.0], [-1.0, 3.0], [0.0, 0.0]])


def test_round_trip_on_interior_values():
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(0)
    Y = np.stack([np.exp(rng.normal(0, 3, 500)), rng.uniform(-0.999, 2.999, 500), rng.normal(0, 10, 500)], axis=1)
    T = abcutil.transform_params(Y, KINDS, BOUNDS)
    assert np.all(np.isfinite(T))
    assert np.array_equal(T[:, 0], np.log(Y[:, 0]))
    assert np.array_equal(T[:, 1], np.log((Y[:, 1] + 1.0) / (3.0 - Y[:, 1])))
    back = abcutil.untransform_params(T, KINDS, BOUNDS)
    # log: exp(log y) within 2 |t| + 1 ulps of y at most; the logit's derivative is bounded by (hi - lo) / 4
    assert np.all(np.abs(back[:, 0] - Y[:, 0]) <= (2 * np.abs(T[:, 0]) + 2) * np.spacing(Y[:, 0]))
    assert np.all(np.abs(back[:, 1] - Y[:, 1]) <= (np.abs(T[:, 1]) + 4) * 2.0 ** -52 * 4.0)
    assert np.array_equal(back[:, 2].view(np.uint64), Y[:, 2].view(np.uint64))


def test_out_of_domain_is_nan():
    from abcsmc_amd import abcutil
    bad = np.array([0.0, -0.0, -1.0, -1e-300, np.inf, -np.inf, np.nan])
    T = abcutil.transform_params(np.stack([bad, bad, bad], axis=1), KINDS, BOUNDS)
    assert np.isnan(T[:, 0]).all()                                       # y <= 0 and non-finite y; 0 is NaN, not -inf
    edge = np.array([-1.0, 3.0, -1.0000000000000002, 3.0000000000000004, np.inf, -np.inf, np.nan])
    T = abcutil.transform_params(np.stack([np.ones(7), edge, np.ones(7)], axis=1), KINDS, BOUNDS)
    assert np.isnan(T[:, 1]).all() and np.all(T[:, 0] == 0.0) and np.all(T[:, 2] == 1.0)
    inside = np.array([np.nextafter(-1.0, 0.0), np.nextafter(3.0, 0.0)])
    T = abcutil.transform_params(np.stack([np.ones(2), inside, np.ones(2)], axis=1), KINDS, BOUNDS)
    assert np.all(np.isfinite(T[:, 1])) and T[0, 1] < -30 and T[1, 1] > 30


def test_none_is_bit_identical():
    from abcsmc_amd import abcutil
    v = np.array([-0.0, 0.0, np.nan, -np.inf, np.inf, 5e-324, -1.5])
    v[2] = np.frombuffer(np.uint64(0x7FF8000000000123).tobytes(), dtype=np.float64)[0]        # a NaN with a payload
    Y = np.stack([np.ones(7), np.ones(7), v], axis=1)
    for fn in (abcutil.transform_params, abcutil.untransform_params):
        out = fn(Y, KINDS, BOUNDS)
        assert np.array_equal(out[:, 2].view(np.uint64), v.view(np.uint64))
    assert np.signbit(abcutil.transform_params(Y, KINDS, BOUNDS)[0, 2])


def test_back_logit_stays_within_bounds_and_nan_stays_nan():
    from abcsmc_amd import abcutil
    t = np.array([0.0, 1.0, 40.0, 800.0, np.inf])
    t = np.concatenate([t, -t])
    for lo, hi in ((-1.0, 3.0), (0.0, 1.0), (0.1, 0.30000000000000004), (-1e300, 1e300), (1.0, np.nextafter(1.0, 2.0))):
        b = np.array([[lo, hi]])
        y = abcutil.untransform_params(t[:, None], ["logit"], b)[:, 0]
        assert np.all((y >= lo) & (y <= hi)), (lo, hi, y)
        assert y[4] == hi and y[9] == lo                                 # t = +inf gives hi, t = -inf gives lo
        assert np.all(np.diff(y[:5]) >= 0) and np.all(np.diff(y[5:]) <= 0)
    nan = np.full((3, 3), np.nan)
    assert np.isnan(abcutil.untransform_params(nan, KINDS, BOUNDS)).all()
    assert np.isnan(abcutil.transform_params(nan, KINDS, BOUNDS)).all()
    assert abcutil.untransform_params(np.array([[-np.inf, 0.0, 0.0]]), KINDS, BOUNDS)[0, 0] == 0.0     # exp(-inf)


def test_arguments():
    from abcsmc_amd import abcutil
    Y = np.ones((4, 3))
    with pytest.raises(ValueError):
        abcutil.transform_params(Y, ("log", "none"), None)               # one entry per parameter
    with pytest.raises(ValueError):
        abcutil.transform_params(Y, ("log", "logit", "none"), None)      # logit needs bounds
    with pytest.raises(ValueError):
        abcutil.transform_params(Y, ("log", "probit", "none"), BOUNDS)
    assert np.array_equal(abcutil.transform_params(Y, ("log", "none", "none")), np.stack([np.zeros(4), np.ones(4), np.ones(4)], 1))


def _support_case(K, nc, P, seed, kind, lo=0.0, hi=1.0):
    """K retained rows of nc fabricated scores in ranking order around the observation o, and P parameters made as the
    back-transform of (linear in the scores + noise): positive under "log", inside (lo, hi) under "logit" """
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((K, nc))
    o = np.full(nc, 0.25)
    d = np.sqrt(((S - o) ** 2).sum(axis=1))
    order = np.argsort(d, kind="stable")
    S, d = S[order], d[order]
    eta = S @ rng.normal(0.0, 1.2, (nc, P)) + 0.3 * rng.standard_normal((K, P))
    theta = np.exp(eta) if kind == "log" else lo + (hi - lo) / (1.0 + np.exp(-1.5 * eta))
    return d, S, o, theta


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("K,nc,P,kind,lo,hi", [(257, 3, 4, "log", 0.0, np.inf), (1000, 4, 6, "logit", -1.0, 3.0)])
def test_plain_regression_leaves_the_support_and_the_transformed_one_does_not(kernel, K, nc, P, kind, lo, hi):
    """the motivating case, for the reference regression alone (the GPU test of the support rests on it)"""
    from abcsmc_amd import abcutil
    d, S, o, theta = _support_case(K, nc, P, 11, kind, lo, hi)
    assert np.all((theta > lo) & (theta < hi))
    plain = R.loclinear(d, S, o, theta, kernel=kernel)
    w = plain["weight"] > 0
    outside = (plain["theta"][w] <= lo) | (plain["theta"][w] >= hi)
    assert outside.sum() > 0, "the plain adjustment stays inside the support: the case shows nothing"
    kinds, bounds = [kind] * P, (None if kind == "log" else np.tile([lo, hi], (P, 1)))
    t = abcutil.transform_params(theta, kinds, bounds)
    fit = R.loclinear(d, S, o, t, kernel=kernel)
    back = abcutil.untransform_params(fit["theta"], kinds, bounds)
    assert np.all(np.isfinite(back))
    if kind == "log":
        assert np.all(back > 0.0)
    else:
        assert np.all((back >= lo) & (back <= hi)) and np.all((back[w] > lo) & (back[w] < hi))
    assert np.array_equal(fit["weight"], plain["weight"])                # the weights do not change


def test_keywords_are_forwarded_only_when_given(monkeypatch):
    from abcsmc_amd import abcutil
    N, M, P, n = 100, 3, 2, 10
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((N, M)), np.exp(rng.standard_normal((N, P)))
    seen = {}

    def fake_new(Xa, Ya, T, f, K, exclude=None, kernel="epanechnikov", max_comp=0, rule=0, theta=True, ctx=None, transf=None,
                 bounds=None):
        seen.update(transf=transf, bounds=bounds)
        coef = np.zeros((len(exclude), 3, P))
        return dict(idx=np.zeros((len(exclude), K), np.uint64), coef=coef, post_mean=coef[:, 0] + 1.0, ncomp=1)

    def fake_old(Xa, Ya, T, f, K, exclude=None, kernel="epanechnikov", max_comp=0, rule=0, theta=True, ctx=None):
        seen["old"] = True
        coef = np.zeros((len(exclude), 3, P))
        return dict(idx=np.zeros((len(exclude), K), np.uint64), coef=coef, post_mean=coef[:, 0] + 1.0, ncomp=1)

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_adjust", fake_new)
    b = [[0, 1], [0, 0]]
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear", transf=("logit", "log"), bounds=b)
    assert seen["transf"] == ("logit", "log") and seen["bounds"] == b
    abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear", transf=("none", "log"))
    assert seen["transf"] == ("none", "log") and seen["bounds"] is None
    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_adjust", fake_old)
    cv = abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear")     # today's signature: the default call reaches it
    assert seen["old"] and np.all(cv["post_mean"] == 1.0)
    with pytest.raises(TypeError):
        abcutil.cross_validate_pls(X, Y, n, 7, seed=4, method="loclinear", transf=("log", "log"))

    def fake_path(Xa, Ya, T, f, Ks, kernel="epanechnikov", exclude=None, max_comp=0, rule=0, ctx=None, **kw):
        seen["path_kw"] = kw
        B, nt = len(exclude), len(Ks)
        z = np.zeros((B, nt, P))
        return dict(post_mean=z, alpha=z + 2.0, Ks=np.asarray(Ks), idx=np.zeros((B, Ks[-1]), np.uint64), ncomp=1,
                    **({"alpha_back": z + 3.0} if kw else {}))

    monkeypatch.setattr(abcutil, "particle_ranking_PLS_targets_path", fake_path)
    cv = abcutil.cross_validate_pls_path(X, Y, n, (3, 7), seed=4, method="loclinear")
    assert seen["path_kw"] == {} and np.all(cv["post_mean"] == 2.0)
    cv = abcutil.cross_validate_pls_path(X, Y, n, (3, 7), seed=4, method="loclinear", transf=("log", "log"))
    assert seen["path_kw"] == {"transf": ("log", "log")} and np.all(cv["post_mean"] == 3.0)
