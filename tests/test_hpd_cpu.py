"""The highest-density intervals without a GPU: the NumPy reference of the header's definition (tests/_hpd_ref.py) against a
brute-force minimisation, against coda::HPDinterval's rule, on the degenerate and the tie rule; the C ABI's declarations, the
bindings and the wrappers."""
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _hpd_ref as H
import _summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("abc_rank_targets_hpd_dev", "abc_particle_ranking_pls_targets_hpd", "abc_weighted_hpd_dev", "abc_weighted_hpd")
LD = np.longdouble


def _samples(ns=(2, 3, 5, 17, 64, 257)):
    rng = np.random.default_rng(1)
    for n in ns:
        for kind in ("gamma", "normal", "ties"):
            v = rng.gamma(2.0, size=n) if kind == "gamma" else rng.normal(size=n)
            if kind == "ties":
                v = np.round(v * 2.0) / 2.0
            for w in (None, rng.uniform(0.1, 1.0, size=n)):
                yield v, w


@pytest.mark.parametrize("m", [0.05, 0.5, 0.9, 0.95])
def test_reference_against_brute_force(m):
    """min over p in [p_0, p_{n-1} - m] of Q(p + m) - Q(p) in long double, on 300 grid points plus every breakpoint (p_r and
    p_r - m inside the range): the reference's width is not above the brute-force minimum, and it is one of the minimisers.  Both
    evaluate the same piecewise-linear function in long double and the reference returns its ends as float64, so the two widths
    may differ by the rounding of two float64 ends: 4 x 2^-53 of the largest |value|."""
    for v, w in _samples((2, 3, 5, 17, 64)):
        u, om = R.sorted_segment(v, w)
        p, _ = R.knots(om, LD)
        lo, hi, plo, phi, _margin = H.hpd_segment(v, w, (m,), LD)
        a, b = p[0], p[-1] - LD(m)
        if not a <= b:                                         # m beyond the span: the degenerate rule
            assert (lo[0], hi[0]) == (u[0], u[-1])
            continue
        grid = np.concatenate([a + (b - a) * np.linspace(0, 1, 300).astype(LD), p, p - LD(m)])
        grid = grid[(grid >= a) & (grid <= b)]
        wd = np.array([R.quantile_sorted(u, p, g + LD(m), LD) - R.quantile_sorted(u, p, g, LD) for g in grid])
        tol = 4 * 2.0 ** -53 * float(np.max(np.abs(u)))
        assert hi[0] - lo[0] <= wd.min() + tol, (u.size, m, hi[0] - lo[0], wd.min())
        assert hi[0] - lo[0] >= wd.min() - tol                 # (every candidate is a grid point: it is a minimiser)
        assert p[0] - 1e-15 <= plo[0] and phi[0] <= p[-1] + 1e-15 and abs((phi[0] - plo[0]) - m) <= 1e-15


def test_fast_reference_is_the_literal_one():
    for v, w in _samples():
        for m in (1e-6, 0.3, 0.5, 0.95, 1 - 1e-9):
            lit = H.hpd_literal(v, w, m)
            fast = H.hpd_segment(v, w, (m,))
            assert all(np.array_equal(fast[k][0], lit[k]) and np.signbit(fast[k][0]) == np.signbit(lit[k]) for k in range(4)), (v.size, m)


@pytest.mark.parametrize("n,m", [(2, 0.5), (64, 0.5), (100, 0.5), (100, 0.9), (100, 0.95), (1000, 0.5), (1000, 0.9), (1000, 0.95)])
def test_reference_against_coda_rule(n, m):
    """equal weights, integer n m (the pairs of n in {2, 3, 5, 64, 100, 1000} and m in {0.5, 0.9, 0.95} for which it is one): coda's
    interval [x_i, x_{i + n m}].  The ends fall on knots up to the rounding of p_r + m, so the interval agrees within 1e-12 of the
    range"""
    rng = np.random.default_rng(n)
    for _ in range(10):
        v = rng.gamma(2.0, size=n)
        lo, hi, _plo, _phi = H.hpd_segment(v, None, (m,))
        clo, chi = H.coda_interval(v, m)
        tol = 1e-12 * (v.max() - v.min())
        assert abs(lo[0] - clo) <= tol and abs(hi[0] - chi) <= tol, (n, m, lo[0], hi[0], clo, chi)


def test_degenerate_rule():
    lo, hi, plo, phi = H.hpd_segment([3.5], None, (0.5, 0.95))
    assert np.array_equal(lo, [3.5, 3.5]) and np.array_equal(hi, [3.5, 3.5]) and np.array_equal(plo, [0.5, 0.5]) and np.array_equal(phi, [0.5, 0.5])
    v = np.array([4.0, 1.0, 2.0, 8.0])                          # knots 1/8 .. 7/8: span 0.75
    for m in (0.75 + 1e-12, 0.8, 1 - 1e-9):
        lo, hi, plo, phi = H.hpd_segment(v, None, (m,))
        assert (lo[0], hi[0], plo[0], phi[0]) == (1.0, 8.0, 0.125, 0.875)
        assert H.hpd_literal(v, None, m) == (1.0, 8.0, 0.125, 0.875, -1)
    assert H.hpd_literal(v, None, 0.75)[:4] == (1.0, 8.0, 0.125, 0.875)     # exactly the span: candidate 0 is valid and says the same
    assert H.hpd_literal(v, None, 0.75)[4] == 0
    assert all(np.isnan(x).all() for x in H.hpd_segment([1.0, np.inf, 2.0], None, (0.5,)))
    assert all(np.isnan(x).all() for x in H.hpd_segment([1.0, 2.0], [0.0, 0.0], (0.5,)))


def test_tie_rule():
    v = np.full(9, 2.5)
    for w in (None, np.linspace(0.2, 1.0, 9)):
        lo, hi, plo, phi, c = H.hpd_literal(v, w, 0.5)
        p, _ = R.knots(R.sorted_segment(v, w)[1])
        assert (lo, hi) == (2.5, 2.5) and c == 0 and plo == p[0] and phi == p[0] + 0.5    # width 0 everywhere: the smallest valid c
    # the smallest VALID one: with m = 0.9 no kind-0 candidate but r = 0 is valid, and c = 0 still wins over the kind-1 ones
    lo, hi, plo, phi, c = H.hpd_literal(np.full(20, -1.0), None, 0.9)
    assert c == 0 and (lo, hi) == (-1.0, -1.0)
    # two separated clusters of equal width: the first in c's order
    v = np.array([0.0, 1.0, 10.0, 11.0])
    lo, hi, plo, phi, c = H.hpd_literal(v, None, 0.25)
    assert (lo, hi, c) == (0.0, 1.0, 0)


def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % re.escape(name), hdr)
    assert m, name + " is not declared in the header"
    return [a.strip() for a in m.group(1).split(",")]


def test_abi_entries_declared_exported_and_bound():
    from abcsmc_amd import _lib
    for n in ENTRIES:
        summ = n.replace("hpd", "summary")
        assert len(_header_args(n)) == len(_header_args(summ)), n
        assert n in _lib.SIGNATURES and _lib.SIGNATURES[n] == _lib.SIGNATURES[summ], n
    pats = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "abcsmc_amd", "csrc", "exports.map")).read())
    assert all(any(fnmatch.fnmatchcase(n, p.strip()) for p in pats) for n in ENTRIES)
    hdr = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} abc_hpd;", hdr)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["mass", "nm", "lo", "hi", "plo", "phi"] == [f[0] for f in _lib.Hpd._fields_]
    assert "NOT been compared with R" in hdr                                # (coda: the header says so)
    assert "hpd" not in _lib.PRODUCTS and len(_lib.PRODUCTS) == 4           # (the four earlier products' list stays as it is)


def test_python_wrappers_exist():
    from abcsmc_amd import abcutil, device, hpd
    ps = inspect.signature(abcutil.particle_ranking_PLS_targets_hpd).parameters
    assert ps["mass"].default == (0.5, 0.95)
    for k in ("method", "kernel", "transf", "bounds", "hcorr", "ridge", "row_weights"):
        assert k in ps, k
    ps = inspect.signature(abcutil.weighted_hpd).parameters
    assert list(ps)[:3] == ["values", "weights", "mass"] and ps["mass"].default == (0.95,)
    assert abcutil.weighted_hpd is hpd.weighted_hpd
    assert callable(device.rank_targets_hpd) and callable(device.weighted_hpd)
    assert inspect.signature(abcutil.cross_validate_pls).parameters["hpd"].default is None


def test_facade_compiles():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "void f() {\n"
           "  ABC::Mat2D X(9, 2), Y(9, 3), T(2, 2);\n"
           "  std::vector<ABC::TargetHpd> r = ABC::particle_ranking_PLS_targets_hpd(X, Y, T, 0.5f, 6);\n"
           "  std::vector<ABC::TargetHpd> s = ABC::particle_ranking_PLS_targets_hpd(X, Y, T, 0.5f, 6, {0.9}, 1, 1);\n"
           "  ABC::TargetHpd g = ABC::weighted_hpd(Y), h = ABC::weighted_hpd(Y, std::vector<double>(9, 1.0), {0.5, 0.9});\n"
           "  double v = r[0].lo(0, 0) + s[0].hi(0, 1) + g.plo(0, 0) + h.phi(1, 2); (void)v;\n"
           "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
