"""CPU: the facts the summaries along a tolerance path rest on (tests/_path_summary_ref.py) and the new surfaces (no GPU call).
The list sorted once at K_max and filtered by e < K_t is the sorted segment of the prefix; the integer form of the knots gives
_summary_ref's bits; rows past a tolerance never reach it; coverage_ks on hand-made values; the bindings and arguments."""
import fnmatch
import os
import re

import numpy as np
import pytest

import _path_summary_ref as PS
import _summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("abc_rank_targets_path_summary_dev", "abc_particle_ranking_pls_targets_path_summary")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _cases():
    rng = np.random.default_rng(3)
    ties = rng.integers(-3, 4, 600).astype(np.float64) / 2.0                  # 7 distinct values: every cut falls inside a run of ties
    zeros = np.where(rng.integers(0, 2, 600) == 0, -0.0, 0.0)                 # signed zeros only
    mixed = rng.integers(-1, 2, 600).astype(np.float64)                       # -1, -0.0, +0.0, 1
    mixed[::7] = -0.0
    mixed[3::7] = 0.0
    smooth = rng.standard_normal(600)
    far = rng.standard_normal(600)
    far[300], far[410], far[520], far[599] = np.inf, -np.inf, np.nan, -np.nan
    return dict(ties=ties, zeros=zeros, mixed=mixed, smooth=smooth, far=far)


KS = (1, 2, 3, 7, 100, 256, 257, 300, 301, 411, 600)


@pytest.mark.parametrize("name", ["ties", "zeros", "mixed", "smooth", "far"])
def test_filtered_shared_sort_is_the_prefix_sort(name):
    v = _cases()[name]
    for (u, e), K in zip(PS.shared_sort(v, KS), KS):
        ur, _ = R.sorted_segment(v[:K])
        assert u.size == K and np.array_equal(_bits(u), _bits(ur)), (name, K)          # bits: -0.0 before +0.0, NaN payloads
        assert np.array_equal(np.sort(e), np.arange(K))
        same = _bits(u)[1:] == _bits(u)[:-1]
        assert np.all(e[1:][same] > e[:-1][same]), (name, K)                          # ties by entry number
    if name in ("ties", "zeros", "mixed"):                                            # the cuts do straddle runs of ties
        assert all(np.any(_bits(v[K:]) == _bits(v[K - 1])) for K in KS[:-1])


@pytest.mark.parametrize("threads,per", [(512, 16), (8, 4)])
def test_walk_from_the_largest_tolerance_down(threads, per):
    """the kernels' order of work (compaction in place, tile by tile: several tiles with 8 x 4 entries) leaves at every tolerance
    the filtered list"""
    for name, v in _cases().items():
        for Ks in (KS, (600,), (1, 600), (32, 33, 64, 65, 599, 600)):
            for (u, e), (uw, ew) in zip(PS.shared_sort(v, Ks), PS.walk_down(v, Ks, threads, per)):
                assert np.array_equal(_bits(u), _bits(uw)) and np.array_equal(e, ew), (name, Ks)


@pytest.mark.parametrize("K", [1, 2, 3, 7, 256, 257])
def test_integer_knots_give_the_reference_bits(K):
    rng = np.random.default_rng(K)
    for v in (rng.standard_normal(K), np.round(rng.standard_normal(K) * 2.0) / 2.0):
        u, om = R.sorted_segment(v)
        p, W = R.knots(om)
        on_knots = [(r + 0.5) / K for r in sorted({0, K // 3, K // 2, K - 1})]
        between = [float(np.nextafter(x, s)) for x in on_knots for s in (0.0, 1.0)]
        probs = [0.0, 1.0, 0.025, 0.5, 0.975, 0.3] + on_knots + [min(1.0, max(0.0, x)) for x in between]
        assert np.array_equal(_bits(p), _bits((np.arange(K) + 0.5) / K)) and W == K
        for q in probs:
            a, b = PS.quantile_int(u, q), R.quantile_sorted(u, p, q)
            assert np.array_equal(_bits(a), _bits(b)), (K, q, a, b)
        for tau in (u[0], u[K // 2], u[-1], u[0] - 1.0, u[-1] + 1.0, 0.0, -0.0, np.inf, -np.inf, np.nan):
            a, b = PS.cdf_int(u, tau), R.cdf_sorted(u, om, W, tau)
            assert np.array_equal(_bits(a), _bits(b)), (K, tau, a, b)


def test_shared_evaluation_is_the_summary_of_every_prefix():
    probs = (0.025, 0.5, 0.975, 0.0, 1.0, 0.3)
    for name, v in _cases().items():
        for tau in (v[3], 0.0, 0.25, np.nan):
            q, c = PS.summary_shared(v, KS, probs, tau)
            qr, cr = PS.path_summary(v, KS, probs, tau)
            assert np.array_equal(_bits(q), _bits(qr)), name
            assert np.array_equal(np.isnan(c), np.isnan(cr)) and np.array_equal(c[~np.isnan(c)], cr[~np.isnan(cr)]), (name, tau)


def test_farther_rows_stay_out():
    v = _cases()["far"]                                   # inf at 300, -inf at 410, NaN at 520 and 599
    q, c = PS.path_summary(v, KS, truth=0.1)
    clean = v.copy()
    clean[[300, 410, 520, 599]] = 0.0
    q0, c0 = PS.path_summary(clean, KS, truth=0.1)
    for t, K in enumerate(KS):
        if K <= 300:
            assert np.array_equal(_bits(q[t]), _bits(q0[t])) and c[t] == c0[t] and np.all(np.isfinite(q[t]))
        else:
            assert np.all(np.isnan(q[t])) and np.isnan(c[t])


def test_coverage_ks():
    from abcsmc_amd.abcutil import coverage_ks
    assert coverage_ks(np.array([0.5])) == 0.5
    assert coverage_ks(np.array([0.25, 0.75])) == 0.25
    assert coverage_ks(np.zeros(4)) == 1.0 and coverage_ks(np.ones(4)) == 1.0
    m = 8
    assert coverage_ks((np.arange(m) + 0.5) / m) == 0.5 / m                   # the best m values can do
    assert coverage_ks(np.array([0.1, 0.2, 0.3])) == pytest.approx(0.7)       # F_n = 1 from 0.3 on
    assert coverage_ks(np.array([np.nan, 0.5, np.inf])) == 0.5                # finite values only
    u = np.full((3, 2, 2), np.nan)
    u[:, 0, 0] = (0.25, 0.75, np.nan)
    u[:, 1, 1] = 0.0
    ks = coverage_ks(u)
    assert ks.shape == (2, 2) and ks[0, 0] == 0.25 and ks[1, 1] == 1.0 and np.isnan(ks[0, 1]) and np.isnan(ks[1, 0])


def test_cross_validate_pls_path_arguments():
    from abcsmc_amd import abcutil
    X, Y = np.zeros((10, 2)), np.zeros((10, 2))
    with pytest.raises(ValueError, match="statistic"):
        abcutil.cross_validate_pls_path(X, Y, 3, (2, 4), seed=1, statistic="mode")
    with pytest.raises(ValueError, match="statistic"):
        abcutil.cross_validate_pls_path(X, Y, 3, (2, 4), seed=1, statistic="nonsense", coverage=True)
    with pytest.raises(ValueError, match="method"):
        abcutil.cross_validate_pls_path(X, Y, 3, (2, 4), seed=1, method="ridge", statistic="median")


def test_header_exports_and_bindings_agree():
    hdr = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    exports = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", exports)
    from abcsmc_amd import _lib, abcutil, device
    for name, nargs in zip(NAMES, (20, 19)):
        m = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert "const abc_path* path" in m.group(1) and "const abc_summary* sum" in m.group(1)
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in pats), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "B x T x nq x P" in hdr and "[b][t][q][j]" in hdr
    assert len(_lib.PRODUCTS) == 4
    assert callable(abcutil.particle_ranking_PLS_targets_path_summary) and callable(device.rank_targets_path_summary)
    assert callable(abcutil.coverage_ks)
