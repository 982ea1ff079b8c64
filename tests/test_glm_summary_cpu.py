"""CPU: the reference of the exact CDF and quantiles of the ABC-GLM marginals (tests/_glm_summary_ref.py) against hand-worked
cases and the bracket inequality, the restated device iteration against that reference, the declarations of the four *_summary
entries, and cross_validate_pls_glm's coverage through a NumPy stand-in.  No GPU call."""
import fnmatch
import math
import os
import re

import numpy as np
import pytest

import _glm_cases as GC
import _glm_ref as R
import _glm_summary_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("abc_glm_rank_targets_summary_dev", "abc_glm_particle_ranking_pls_targets_summary", "abc_glm_weighted_summary_dev",
         "abc_glm_weighted_summary")
LEVELS = (1e-6, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0 - 1e-6)


def mixture(K, loc, sigma, seed, bimodal=False):
    """K peaks about loc with spread 3 sigma (bimodal: two groups 80 sigma apart), 1/7 of the weights zero"""
    rng = np.random.default_rng(seed)
    t = loc + 3.0 * sigma * rng.normal(size=K)
    if bimodal:
        t[:K // 2] -= 40.0 * sigma
        t[K // 2:] += 40.0 * sigma
    c = rng.uniform(0.1, 1.0, size=K)
    if K > 7:
        c[::7] = 0.0
    return t, c / c.sum(), sigma


MIXTURES = {"k37": (37, 0.3, 0.5, 1, False), "k2000": (2000, 1e3, 3e-3, 2, False), "k5000_bimodal": (5000, 0.0, 1.0, 3, True),
            "k257_far": (257, 1e6, 3e-4, 4, False)}


def test_one_peak():
    """Q(q) = t + sigma z_q and F(t) = 1/2"""
    t, c, sigma = [1.25], [1.0], 0.75
    assert S.F_ref(1.25, t, c, sigma) == 0.5
    for q in LEVELS:
        x = S.Q_ref(q, t, c, sigma)
        want = 1.25 + sigma * S.z_of(q)
        # z_q is good to a few ulps; near the ends F is flat, so the root is known to what q's own rounding is worth in x
        slack = 8 * np.spacing(abs(want)) + 2.0 ** -52 / S.f_ref(want, t, c, sigma)
        assert abs(x - want) <= slack, (q, x, want)


def test_two_equal_peaks_have_their_median_in_the_middle():
    t, c, sigma = [-3.0, 5.0], [0.5, 0.5], 0.5
    assert abs(S.F_ref(1.0, t, c, sigma) - 0.5) <= 2.0 ** -53
    x = S.Q_ref(0.5, t, c, sigma)
    # the density in the gap is about 1e-14, so F is flat there to rounding: the median is held to F, and lies in the gap
    assert -3.0 < x < 5.0 and abs(S.F_ref(x, t, c, sigma) - 0.5) <= S.quant_bound(x, t, c, sigma)
    t = [0.0, 1.0]                                              # overlapping peaks: the median is the midpoint
    x = S.Q_ref(0.5, t, c, sigma)
    assert abs(x - 0.5) <= 4 * np.spacing(0.5), x


@pytest.mark.parametrize("name", sorted(MIXTURES))
def test_reference_inverts_itself_and_the_bracket_holds(name):
    t, c, sigma = mixture(*MIXTURES[name])
    tl, cl = S.counted(t, c)
    worst = 0.0
    for q in LEVELS:
        x = S.Q_ref(q, tl, cl, sigma)
        res = abs(S.F_ref(x, tl, cl, sigma) - q) / S.quant_bound(x, tl, cl, sigma)
        worst = max(worst, res)
        assert res <= 1.0, (q, res)
        lo, hi = S.bracket(tl, sigma, q)
        assert lo <= x <= hi, (q, lo, x, hi)
    print(name, "worst residual %.3f of the bound" % worst)
    # Phi((x - t_max) / sigma) <= F(x) <= Phi((x - t_min) / sigma) wherever x is
    rng = np.random.default_rng(5)
    for x in rng.uniform(min(tl) - 6 * sigma, max(tl) + 6 * sigma, size=25):
        F = S.F_ref(x, tl, cl, sigma)
        W = math.fsum(cl)
        assert W * S.F_ref(x, [max(tl)], [1.0], sigma) * (1 - 1e-14) <= F <= W * S.F_ref(x, [min(tl)], [1.0], sigma) * (1 + 1e-14), x


@pytest.mark.parametrize("name", sorted(MIXTURES))
def test_restated_device_iteration_meets_the_bound_within_its_cap(name):
    """the kernel's safeguarded Newton iteration in plain fp64 (a fp64 sum, not fsum): F_ref of its result within the GPU test's
    bar, and it ends on its bracket, not on its cap"""
    t, c, sigma = mixture(*MIXTURES[name])
    tl, cl = S.counted(t, c)
    its = []
    for q in LEVELS + (1e-9, 1.0 - 1e-9):
        x, it = S.newton_model(q, np.array(tl), np.array(cl), sigma)
        its.append(it)
        assert it < S.QCAP, (q, it)
        res = abs(S.F_ref(x, tl, cl, sigma) - q) / S.quant_bound(x, tl, cl, sigma)
        assert res <= 1.0, (q, res)
    print(name, "iterations per level", its)


def test_the_four_entries_are_declared_bound_and_exported():
    from abcsmc_amd import _lib
    txt = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    old = {"abc_glm_rank_targets_summary_dev": "abc_glm_rank_targets_dev",
           "abc_glm_particle_ranking_pls_targets_summary": "abc_glm_particle_ranking_pls_targets",
           "abc_glm_weighted_summary_dev": "abc_glm_weighted_dev", "abc_glm_weighted_summary": "abc_glm_weighted"}
    patterns = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "abcsmc_amd", "csrc", "exports.map")).read())
    patterns = [p.strip() for g in patterns for p in g.split()]
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, "%s is not declared" % name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        # both descriptors in front of the context, then the arguments of the entry it extends
        assert params[:3] == ["const abc_glm* glm", "const abc_summary* sum", "abc_ctx* ctx"], (name, params[:3])
        base = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % old[name], txt)
        assert params[3:] == [" ".join(p.split()) for p in base.group(1).split(",")][2:], name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        bres, bargs = _lib.SIGNATURES[old[name]]
        assert res is bres and list(args) == [args[0]] + list(bargs), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
    # abc_glm itself is what it was: sixteen outputs behind G, cut, bw_scale and bw
    assert len(_lib.GLM_OUTPUTS) == 16 and len(_lib.Glm._fields_) == 20


def test_python_refuses_levels_and_truths_before_the_library():
    from abcsmc_amd import glm
    th, st = np.zeros((6, 2)), np.zeros((6, 1))
    for bad in ([0.0], [1.0], [-0.1], [float("nan")], [0.5, 1.0], [], np.linspace(0.01, 0.99, 65)):
        with pytest.raises(ValueError):
            glm.weighted_glm(th, st, [0.0], probs=bad)
    with pytest.raises(ValueError):
        glm.weighted_glm(th, st, [0.0], truth=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        glm.cross_validate_pls_glm(np.zeros((9, 2)), np.zeros((9, 2)), 3, 4, 1, statistic="median", probs=[1.5],
                                   posterior=lambda *a, **k: None)
    with pytest.raises(ValueError):
        glm.cross_validate_pls_glm(np.zeros((9, 2)), np.zeros((9, 2)), 3, 4, 1, statistic="mean-ish", posterior=lambda *a, **k: None)


@pytest.fixture(scope="module")
def table():
    from abcsmc_amd import synthetic
    return synthetic.Workload(8, 4).rows(0, 2000)


def test_cross_validation_defaults_hand_the_stand_in_what_they_did(oracle, table):
    from abcsmc_amd import glm
    X, Y = table
    post = S.numpy_posterior(oracle, R, GC)
    cv = glm.cross_validate_pls_glm(X, Y, 5, 60, seed=3, posterior=post)
    assert len(post.calls) == 1
    kw = post.calls[0]
    assert sorted(kw) == ["bw_scale", "ctx", "exclude", "max_comp", "outputs", "rule"]
    assert kw["outputs"] == ("mean", "log_md", "status") and np.array_equal(kw["exclude"], cv["rows"])
    assert sorted(cv) == ["idx", "log_md", "ncomp", "post_mean", "pred_error", "rows", "status", "theta"]


def test_cross_validation_coverage_and_median(oracle, table):
    from abcsmc_amd import abcutil, glm
    X, Y = table
    n, K, P = 12, 80, Y.shape[1]
    post = S.numpy_posterior(oracle, R, GC)
    cv = glm.cross_validate_pls_glm(X, Y, n, K, seed=3, posterior=post, coverage=True, probs=(0.1, 0.9), statistic="median")
    kw = post.calls[0]
    assert np.array_equal(kw["probs"], [0.1, 0.9, 0.5]) and np.array_equal(kw["truth"], cv["theta"])
    assert kw["outputs"] == ("log_md", "status")
    assert cv["truth_cdf"].shape == (n, P) and cv["ci95"].shape == (P,) and cv["coverage_ks"].shape == (P,)
    assert cv["quant"].shape == (n, 2, P) and cv["post_median"].shape == (n, P) and cv["pred_error"].shape == (P,)
    assert np.all(cv["status"] == 0) and np.all((cv["truth_cdf"] > 0) & (cv["truth_cdf"] < 1))
    assert np.all(cv["quant"][:, 0] < cv["post_median"]) and np.all(cv["post_median"] < cv["quant"][:, 1])
    u = cv["truth_cdf"]
    assert np.array_equal(cv["ci95"], ((u >= 0.025) & (u <= 0.975)).mean(axis=0))
    assert np.array_equal(cv["coverage_ks"], abcutil.coverage_ks(u))
    # the same rows and the same retained sets as without
    plain = glm.cross_validate_pls_glm(X, Y, n, K, seed=3, posterior=post)
    assert np.array_equal(plain["rows"], cv["rows"]) and np.array_equal(plain["idx"], cv["idx"])


def test_ci95_counts_only_the_targets_of_status_zero():
    from abcsmc_amd import glm
    X, Y = np.zeros((10, 2)), np.arange(30.0).reshape(10, 3)
    status = np.array([0, 1, 0, 4, 0, 0])
    cdf = np.array([[0.5, 0.01, 0.975], [np.nan] * 3, [0.025, 0.99, 0.3], [np.nan] * 3, [0.6, 0.5, 0.98], [0.7, 0.2, 0.1]])

    def post(X, Y, T, f, K, **kw):
        return dict(mean=np.zeros((6, 3)), log_md=np.zeros(6), status=status, idx=np.zeros((6, K), dtype=np.int64), ncomp=1,
                    quant=None, cdf=cdf)

    cv = glm.cross_validate_pls_glm(X, Y, 6, 4, seed=1, posterior=post, coverage=True)
    assert np.array_equal(cv["ci95"], [1.0, 0.5, 0.75])       # of the four targets of status 0, not of six
    assert np.array_equal(np.isnan(cv["truth_cdf"]), np.isnan(cdf))


def test_facade_compiles():
    import subprocess
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "void f() {\n"
           "  ABC::Mat2D X(9, 2), Y(9, 3), T(2, 2), truth(2, 3);\n"
           "  std::vector<ABC::TargetGlmSummary> r = ABC::particle_ranking_PLS_targets_glm_summary(X, Y, T, 0.5f, 6, {0.025, 0.5, 0.975});\n"
           "  std::vector<ABC::TargetGlmSummary> s = ABC::particle_ranking_PLS_targets_glm_summary(X, Y, T, 0.5f, 6, {0.5}, truth, 64, 2.0, 1.5);\n"
           "  ABC::TargetGlmSummary g = ABC::weighted_glm_summary(Y, X, ABC::Row(2), {0.5}), h = ABC::weighted_glm_summary(Y, X, ABC::Row(2), {}, ABC::Row(3), std::vector<double>(9, 1.0), 33);\n"
           "  double v = r[0].quant(1, 2) + s[1].cdf[0] + g.glm.log_md + h.cdf[2] + h.glm.status; (void)v;\n"
           "  ABC::TargetGlm old = ABC::weighted_glm(Y, X, ABC::Row(2)); (void)old;\n"
           "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
