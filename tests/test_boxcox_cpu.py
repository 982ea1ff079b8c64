"""CPU: the Box-Cox pre-pass of the metrics (include/abcsmc_hip.h, "Box-Cox transform of the metrics").  The grid's facts through
the long-double reference module (_boxcox_ref) and through abc_box_cox_grid; the definition against the reference implementation's
own double formula where that formula holds, and the column where it does not; the pick rule; the tables of the GPU pick test have
the margins that test relies on; the declarations, bindings and wrappers.  No GPU call."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _boxcox_ref as B
from test_loclinear_cpu import ROOT, _header_args

NEW = {"abc_box_cox_grid": 6, "abc_optimize_box_cox_dev": 9, "abc_optimize_box_cox": 8, "abc_box_cox_dev": 9, "abc_box_cox": 7}
# the tables of the GPU pick test (test_gpu_boxcox.py): (N, M, seed)
PICK_TABLES = ((1000, 7, 11), (4097, 14, 12))
PICK_MARGIN = 2e-9


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- grid ---------------------------------------------------------------------------------------------------------------------------
def test_grid_facts_reference_module():
    g = B.grid()
    assert g.size == 100 and g[0] == -5.0
    assert abs(g[-1] - 4.9000001475) < 1e-9 and g[-1] + float(np.float32(0.1)) > 5.0
    assert not (g == 0).any() and abs(g[50] - 7.45e-8) < 1e-9
    h = B.grid(-2, 2, 0.5)
    assert h.size == 9 and h[4] == 0.0 and _same(h, np.arange(-2.0, 2.25, 0.5))
    assert B.grid(1, 1, 0.1).size == 1


def test_grid_library_agrees_in_count_and_bits():
    from abcsmc_amd import _lib
    for args in ((-5, 5, 0.1), (-2, 2, 0.5), (1, 1, 0.1), (-2.5, 2.5, 0.01), (0.25, 4, 0.3)):
        ref = B.grid(*args)
        assert _same(_lib.box_cox_grid(*args), ref), args
        n = C.c_size_t(7)                                                       # the count alone, without a buffer
        assert _lib.lib().abc_box_cox_grid(*(float(np.float32(a)) for a in args), None, 0, C.byref(n)) == 0 and n.value == ref.size
    small = np.empty(5)
    n = C.c_size_t(0)
    assert _lib.lib().abc_box_cox_grid(-5.0, 5.0, 0.1, small.ctypes.data, 5, C.byref(n)) != 0 and n.value == 100    # cap too small
    for bad in ((-5, 5, 0.0), (-5, 5, -0.1), (5, -5, 0.1), (-5, 5, 0.001), (np.nan, 5, 0.1), (-5, np.inf, 0.1), (-5, 5, np.nan),
                (-5, 5, np.inf)):
        with pytest.raises(ValueError):
            _lib.box_cox_grid(*bad)
    assert _lib.box_cox_grid(0, 5.11, 0.01).size == 512                         # ABC_BOX_COX_MAXL itself is allowed
    with pytest.raises(ValueError):
        _lib.box_cox_grid(0, 5.12, 0.01)


# ---- the definition against the reference implementation's double formula ----------------------------------------------------------------
@pytest.mark.parametrize("family", B.ORDINARY)
def test_definition_matches_reference_double_formula_on_ordinary_columns(family):
    x, shift = B.column(family, 4097, 5)
    g = B.grid()
    sk, st = B.skew_table(x, g, shift)
    rd, rpick = B.reference_double_search(x, g)
    assert st == 0
    err = float(np.max(np.abs(sk - rd)))
    print("%s: max |long-double definition - reference double formula| = %.3g" % (family, err))
    assert err <= 1e-8
    assert B.pick(sk)[0] == rpick


def test_reference_double_formula_is_not_held_on_1000_pm_50():
    """x^-5 - 1 cancels everything at 1000: the reference's own formula is rounding there (measured: off by 1.6 at
    lambda = -5 on this column), the definition is not"""
    x, _ = B.column("wide1000", 4097, 5)
    g = B.grid()
    sk, _ = B.skew_table(x, g)
    rd, _ = B.reference_double_search(x, g)
    err = np.abs(sk - rd).astype(np.float64)
    print("wide1000: |definition - reference double formula| at lambda=-5: %.3g, max %.3g" % (err[0], err.max()))
    assert err.max() > 1e-8
    assert np.all(np.abs(np.diff(sk.astype(np.float64))) < 0.05)                # the definition itself is smooth in lambda


# ---- pick ---------------------------------------------------------------------------------------------------------------------------
def test_pick_rule_on_hand_made_tables():
    nan, inf = np.nan, np.inf
    assert B.pick([3.0, -1.0, 2.0]) == (1, False)
    assert B.pick([1.0, -1.0, 1.0]) == (0, False)                               # a tie keeps the first (strict <)
    assert B.pick([nan, 2.0, -2.0, nan]) == (1, True)
    assert B.pick([nan, nan, nan]) == (0, True)                                 # nothing finite: 0
    assert B.pick([inf, -inf, 5.0]) == (2, True)                                # +-inf is never taken
    assert B.pick([0.0, 0.0]) == (0, False)
    assert B.margin([3.0, -1.0, nan, 1.5]) == 0.5 and B.margin([1.0, -1.0]) == 0.0


def test_status_bits_of_the_reference_module():
    g = B.grid(-2, 2, 0.5)
    r = B.search(np.array([[1.0, 2.0, 3.0], [2.0, 2.0, 0.0], [4.0, 2.0, 5.0]]), g)
    assert list(r["status"]) == [0, B.CONSTANT, B.BAD]
    assert r["pick"][1] == 0 and r["lam"][1] == -2.0 and np.all(r["skew"][1] == 0)
    assert r["pick"][2] == -1 and r["lam"][2] == 1.0 and np.isnan(r["skew"][2].astype(np.float64)).all()
    one = B.search(np.array([[3.0]]), g)                                        # N = 1 is a constant column
    assert one["status"][0] == B.CONSTANT and one["pick"][0] == 0


@pytest.mark.parametrize("N,M,seed", PICK_TABLES)
def test_every_column_of_the_gpu_pick_tables_has_a_margin(N, M, seed):
    X, shift = B.table(N, M, seed)
    r = B.search(X, B.grid(), shift)
    margins = [B.margin(r["skew"][j]) for j in range(M)]
    print("margins:", " ".join("%.2g" % m for m in margins))
    assert min(margins) > PICK_MARGIN and not r["status"].any()


def test_near_tie_column_is_a_near_tie():
    x, g = B.near_tie_column()
    sk, st = B.skew_table(x, g)
    a = np.sort(np.abs(sk.astype(np.float64)))
    pk = B.pick(sk)[0]
    print("near tie: |skew| %.3e vs %.3e at %r, third %.3e" % (a[0], a[1], B.near_tie_indices(sk), a[2]))
    assert st == 0 and a[1] - a[0] < 1e-12 and a[2] - a[1] > 1e-3 and pk in B.near_tie_indices(sk)


# ---- declarations, bindings, wrappers ---------------------------------------------------------------------------------------------------
def test_abi_entries_declared_and_bound():
    from abcsmc_amd import _lib, abcutil, device
    for n, nargs in NEW.items():
        assert len(_header_args(n)) == nargs, n
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n][1]) == nargs, n
    hdr = open(os.path.join(ROOT, "include", "abcsmc_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} abc_box_cox_out;", hdr)
    fields = re.findall(r"\*\s*(\w+);", m.group(1))
    assert fields == ["lambda", "best_skew", "skew", "pick", "status"]
    assert [f[0] for f in _lib.BoxCoxOut._fields_] == ["lam"] + fields[1:]
    assert re.search(r"ABC_BOX_COX_MAXL\s*=\s*512", hdr) and _lib.BOX_COX_MAXL == 512 == B.MAXL
    assert (_lib.BOX_COX_BAD, _lib.BOX_COX_CONSTANT, _lib.BOX_COX_SKIPPED) == (B.BAD, B.CONSTANT, B.SKIPPED)
    for name in ("optimize_box_cox", "box_cox"):
        assert callable(getattr(_lib.Context, name)) and callable(getattr(device, name)) and callable(getattr(abcutil, name))
    ps = inspect.signature(device.optimize_box_cox).parameters
    assert [ps[k].default for k in ("lambda_min", "lambda_max", "step", "shift", "skew", "ctx")] == [-5, 5, 0.1, None, False, None]
    ps = inspect.signature(abcutil.box_cox_metrics).parameters
    assert list(ps) == ["X", "targets", "lambda_min", "lambda_max", "step", "shift", "ctx"]
    assert "boxcox.hip" in open(os.path.join(ROOT, "abcsmc_amd", "csrc", "Makefile")).read()


def test_facade_declares_the_reference_signatures():
    src = ("#include \"abcsmc_amd/cxx/AbcUtilHip.hpp\"\n"
           "void f() {\n"
           "  ABC::Col c{1.0, 2.0, 4.0};\n"
           "  ABC::float_type a = ABC::optimize_box_cox(c);\n"
           "  ABC::float_type b = ABC::optimize_box_cox(c, -2.0f, 2.0f, 0.5f);\n"
           "  ABC::Mat2D X(3, 2);\n"
           "  ABC::Row lam = ABC::optimize_box_cox(X);\n"
           "  ABC::Row lam2 = ABC::optimize_box_cox(X, -2, 2, 0.5f, ABC::Row{1.0, 0.0});\n"
           "  ABC::Mat2D T = ABC::box_cox(X, lam), T2 = ABC::box_cox(X, lam2, ABC::Row{1.0, 0.0});\n"
           "  (void)a; (void)b; (void)T; (void)T2;\n"
           "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-x", "c++", "-"], input=src, text=True,
                       capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "optimize_box_cox" in open(os.path.join(ROOT, "abcsmc_amd", "cxx", "facade_demo.cpp")).read()


def test_abcutil_argument_errors_raise_before_any_context(monkeypatch):
    from abcsmc_amd import abcutil

    def no_context(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(abcutil, "default_context", no_context)
    X = np.abs(np.random.default_rng(0).standard_normal((20, 3))) + 0.1
    for call in (lambda: abcutil.optimize_box_cox(np.empty((0, 3))),
                 lambda: abcutil.optimize_box_cox(np.empty((2, 3, 4))),
                 lambda: abcutil.optimize_box_cox(X, step=0.0),
                 lambda: abcutil.optimize_box_cox(X, lambda_min=1, lambda_max=-1),
                 lambda: abcutil.optimize_box_cox(X, step=0.001),
                 lambda: abcutil.optimize_box_cox(X, shift=[1.0, 2.0]),
                 lambda: abcutil.optimize_box_cox(X, shift=[1.0, np.nan, 0.0]),
                 lambda: abcutil.optimize_box_cox(X, shift="median"),
                 lambda: abcutil.box_cox(X, None),
                 lambda: abcutil.box_cox(X, [1.0, 2.0]),
                 lambda: abcutil.box_cox(X, [1.0, np.inf, 0.0]),
                 lambda: abcutil.box_cox(X, 0.5, shift=[1.0]),
                 lambda: abcutil.box_cox_metrics(X, targets=np.ones((2, 4))),
                 lambda: abcutil.box_cox_metrics(X, targets=np.ones((2, 2, 3))),
                 lambda: abcutil.box_cox_metrics(X, step=-1.0)):
        with pytest.raises(ValueError):
            call()


def test_auto_shift_rule():
    from abcsmc_amd import abcutil
    X = np.asfortranarray(np.array([[1.0, 0.0, -3.5], [2.0, 4.0, 2.0]]))
    assert list(abcutil._box_cox_shift("auto", X)) == [0.0, 1.0, 4.5]
    assert abcutil._box_cox_shift(None, X) is None and list(abcutil._box_cox_shift(2.0, X)) == [2.0, 2.0, 2.0]
