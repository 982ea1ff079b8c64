"""The long-double form of the k-nearest-neighbour posterior entropy (tests/_entropy_ref.py), which the device is held to in
tests/test_gpu_entropy.py, on its own: it agrees with scipy's parts, scales as an entropy does, recovers the entropy of a normal
sample, and follows the header's rules for duplicates and for too few entries.  Then the declarations, bindings and wrappers of the
four entries, and the estimate's use: on the oracle's ranking a target's retained rows have a lower entropy than the table.  No GPU.

Figures of the usefulness test (600 rows of 6 metrics, P = 3, K = 100, k = 4, scale = the columns' standard deviations, 17 targets):
mean entropy of the retained rows 2.5606, entropy of 100 rows taken evenly from the table 4.1521.  The reference against scipy on
a 400 x 5 normal sample differs by at most 1.1e-15, and its worst |H - (3/2) log(2 pi e)| over the twenty normal samples is 0.1195."""
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np

import _entropy_ref as R
from test_loclinear_cpu import ROOT, _header_args

LD = np.longdouble
ENTRIES = ("abc_rank_targets_entropy_dev", "abc_particle_ranking_pls_targets_entropy", "abc_weighted_entropy_dev",
           "abc_weighted_entropy")


# ---- the reference is right ---------------------------------------------------------------------------------------------------
def test_psi_table_is_digamma():
    from scipy.special import digamma, gammaln
    for k in range(1, 9):
        assert abs(float(R.psi(k)) - digamma(k)) <= 4e-16 * max(1.0, abs(digamma(k))), k
    for P in (1, 2, 3, 4, 5, 16, 17, 64, 1023, 1024):
        assert abs(float(R.lgamma_half(P)) - gammaln(0.5 * P + 1)) <= 1e-14 * max(1.0, abs(gammaln(0.5 * P + 1))), P


def test_reference_agrees_with_scipy():
    V = np.random.default_rng(1).standard_normal((400, 5))
    for k in (1, 4, 8):
        h, s = R.entropy(V, k)["H"], R.entropy_scipy(V, k)
        print("k = %d: reference %.15f scipy %.15f difference %.3g" % (k, float(h), s, float(h - LD(s))))
        assert abs(float(h - LD(s))) <= 1e-12
    rho = np.sqrt(R.entropy(V, 4)["rho2"].astype(np.float64))
    from scipy.spatial import cKDTree
    assert np.allclose(rho, cKDTree(V).query(V, k=5)[0][:, 4], rtol=1e-14, atol=0)


def test_scaling_adds_p_log_s():
    V = np.random.default_rng(2).standard_normal((300, 4))
    h = R.entropy(V, 4)["H"]
    for s in (0.5, 3.0, 1024.0):
        assert abs(float(R.entropy(s * V, 4)["H"] - h - 4 * np.log(LD(s)))) <= 1e-12, s
    # and scale divides: scale = 1 / s is the same statement
    assert abs(float(R.entropy(V, 4, scale=np.full(4, 0.25))["H"] - h - 4 * np.log(LD(4)))) <= 1e-12


def test_normal_sample_entropy():
    """the entropy of a standard normal in 3 dimensions is (3 / 2) log(2 pi e); 1000 rows, k = 4, twenty seeds"""
    true = 1.5 * np.log(2 * np.pi * np.e)
    worst = 0.0
    for s in range(20):
        h = float(R.entropy(np.random.default_rng(s).standard_normal((1000, 3)), 4)["H"])
        worst = max(worst, abs(h - true))
    print("worst |H - (3/2) log(2 pi e)| over 20 seeds: %.4f" % worst)
    assert worst <= 0.25


def test_duplicates_and_too_few():
    V = np.random.default_rng(3).standard_normal((50, 3))
    V[7] = V[31]
    r = R.entropy(V, 1)
    assert r["zeros"] == 2 and r["H"] == -np.inf and r["rho2"][7] == 0 and r["rho2"][31] == 0
    r = R.entropy(V, 2)
    assert r["zeros"] == 0 and np.isfinite(r["H"])
    V[40] = V[41] = V[7]                                                   # four copies: zeros up to k = 3
    for k, z in ((1, 4), (3, 4), (4, 0)):
        assert R.entropy(V, k)["zeros"] == z, k
    for K, k in ((4, 4), (3, 4), (1, 1), (8, 8)):
        r = R.entropy(V[10:10 + K], k)
        assert np.isnan(r["H"]) and np.isnan(r["rho2"]).all() and r["zeros"] == 0
    assert np.isfinite(R.entropy(V[10:15], 4)["H"])                        # K = k + 1
    bad = V.copy()
    bad[3, 1] = np.inf
    assert np.isnan(R.entropy(bad, 2)["H"])


# ---- the estimate is useful ---------------------------------------------------------------------------------------------------
def test_retained_rows_are_more_concentrated_than_the_table(oracle):
    """the oracle's ranking of 17 targets: the K = 100 retained rows against 100 rows taken evenly from the whole table"""
    from abcsmc_amd import synthetic
    N, M, P, K = 600, 6, 3, 100
    X, Y = synthetic.Workload(M, P, 40 + P).rows(0, N)
    sd = Y.std(axis=0, ddof=1)
    rows = (np.arange(17) * 31 + 5) % N
    H = [float(R.entropy(Y[oracle.particle_ranking_pls(X, Y, X[r], 0.5)["idx"][:K].astype(np.int64)], 4, sd)["H"]) for r in rows]
    table = float(R.entropy(Y[::N // K], 4, sd)["H"])
    print("mean entropy of the retained rows %.4f, of 100 rows of the table %.4f" % (np.mean(H), table))
    assert np.isfinite(H).all() and np.mean(H) < table


# ---- declarations, bindings, wrappers -----------------------------------------------------------------------------------------
def test_abi_entries_declared_and_bound():
    from abcsmc_amd import _lib
    for n in ENTRIES:
        draws = n.replace("entropy", "draws")
        assert len(_header_args(n)) == len(_header_args(draws)), n
        assert n in _lib.SIGNATURES and _lib.SIGNATURES[n] == _lib.SIGNATURES[draws], n
    pats = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "abcsmc_amd", "csrc", "exports.map")).read())
    assert all(any(fnmatch.fnmatchcase(n, p.strip()) for p in pats) for n in ENTRIES)
    assert len(_lib.PRODUCTS) == 4 and "entropy" not in _lib.PRODUCTS
    hdr = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} abc_entropy;", hdr)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["k", "scale", "H", "knn", "zeros"] == [f[0] for f in _lib.Entropy._fields_]
    assert "NOT been checked against" in hdr                               # (abctools: the header says so)
    assert "entropy.hip" in open(os.path.join(ROOT, "abcsmc_amd", "csrc", "Makefile")).read()


def test_python_wrappers_exist():
    from abcsmc_amd import abcutil, device
    ps = inspect.signature(abcutil.particle_ranking_PLS_targets_entropy).parameters
    assert ps["k"].default == 4 and ps["scale"].default is None
    ps = inspect.signature(abcutil.knn_entropy).parameters
    assert list(ps)[:3] == ["values", "k", "scale"] and ps["k"].default == 4 and ps["scale"].default is None
    assert callable(device.rank_targets_entropy) and callable(device.weighted_entropy)
    ps = inspect.signature(abcutil.cross_validate_pls).parameters
    assert ps["entropy"].default is False
    assert list(inspect.signature(abcutil.min_entropy_components).parameters)[:6] == ["X_orig", "Y_orig", "n_targets", "K", "seed",
                                                                                     "max_comps"]


def test_facade_compiles():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "void f() {\n"
           "  ABC::Mat2D X(9, 2), Y(9, 3), T(2, 2);\n"
           "  std::vector<ABC::TargetEntropy> r = ABC::particle_ranking_PLS_targets_entropy(X, Y, T, 0.5f, 6);\n"
           "  std::vector<ABC::TargetEntropy> s = ABC::particle_ranking_PLS_targets_entropy(X, Y, T, 0.5f, 6, 2, {1.0, 2.0, 3.0}, 1, 1);\n"
           "  ABC::TargetEntropy g = ABC::knn_entropy(Y), h = ABC::knn_entropy(Y, 2, {1.0, 2.0, 3.0});\n"
           "  double H = r[0].H + g.H + h.knn[0]; size_t z = s[0].zeros; (void)H; (void)z;\n"
           "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
