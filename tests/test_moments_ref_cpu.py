"""The host model of the posterior's moments (tests/_moments_ref.py) against itself: the fp64 emulation of the kernels' arithmetic
stays inside the derived bounds E (covariance, dv) and B (factor) at the shapes where the kernels change path, and every wrong
variant lands outside them in the case named for it.  The GPU tests (tests/test_gpu_moments.py) hold the device to the same bounds."""
import numpy as np
import pytest

import _moments_ref as MR


def _collinear(K, P, seed):
    """columns 0 and 1 collinear to 1e-5, means at 10 sd"""
    g = np.random.default_rng(seed)
    th = g.normal(size=(K, P)) + 10.0
    th[:, 1] = th[:, 0] + 1e-5 * g.normal(size=K)
    return th


def _sorted(K, P, seed):
    """Rows sorted by column 0, and two columns that have SETTLED in complementary rows: column P - 2 sits at 0 in the pilot rows
    (0 .. 255) and takes +u, then -u (permuted) below; column P - 1 takes +x, then -x (permuted) in the pilot rows and sits at 0
    below.  With the true pilot (0 for the one, a rounding residue of ~1e-17 for the other) every product of the two columns has
    an exact zero or that residue for a factor, the means are residues too, and E of that covariance entry is ~1e-30: the entry
    is known almost exactly, and the emulation returns it so.  Centred anywhere else (the last 256 rows of column P - 2 average
    about -0.3) the same entry is a cancelling sum of 256 products of size 0.3 |x|, whose rounding, ~1e-16, no longer fits.  The
    other entries cannot tell two centres inside the data apart (both pilots lie about 1 sd from the column mean: the variant's
    shares there are 0.0034 of B, 0.0069 of E, 0.014 of diag(E), the true pilot's 0.0019, 0.0059, 0.0081).  So on ordinary data
    a pilot from the last rows is numerically as good as the true one: the variant is no kernel defect a bound could catch, it
    exercises the shift argument of the helper's bound -- E must be built from the shift the sums were taken about"""
    assert K >= 257 and P >= 3
    th = MR.data("sorted", K, P, seed)
    g = np.random.default_rng(seed + 40)
    nb = K - 256
    u = np.abs(g.normal(size=nb // 2)) + 0.1
    x = np.abs(g.normal(size=128)) + 0.1
    a, b = np.zeros(K), np.zeros(K)
    a[256:256 + nb // 2] = u
    a[256 + nb // 2:256 + 2 * (nb // 2)] = -u[g.permutation(nb // 2)]
    b[:128] = x
    b[128:256] = -x[g.permutation(128)]
    th[:, P - 2], th[:, P - 1] = a, b
    return th


CASES = {
    "benign-300x16": lambda: MR.data("benign", 300, 16, 1),
    "far-300x16": lambda: MR.data("far", 300, 16, 2),
    "collinear-300x8": lambda: _collinear(300, 8, 3),
    "sorted-600x32": lambda: _sorted(600, 32, 4),
    "arena-300x139": lambda: MR.data("benign", 300, 139, 5),
    "tile-257x64": lambda: MR.data("benign", 257, 64, 6),
    "tiny-3x2": lambda: MR.data("benign", 3, 2, 7),
    "tiny-2x1": lambda: MR.data("benign", 2, 1, 8),
}


def _shares(th, **variant):
    """(share of B on the factor, share of E on the strict upper triangle, share of diag(E) on dv, B.max() / max|L|)"""
    em = MR.emulate(th, **variant)
    assert em["ok"]
    sB, sE, E, B, ref = MR.check_factor(em["Lgsl"], th)
    sD = MR.share(np.abs(em["dv"].astype(MR.LD) - np.diag(ref["cov"])).astype(np.float64), np.diag(E))
    return sB, sE, sD, B.max() / np.abs(ref["L"]).max()


@pytest.mark.parametrize("name", list(CASES))
def test_emulation_inside_the_bounds(name):
    sB, sE, sD, rel = _shares(CASES[name]())
    print("%s: share of B %.3g, of E (upper) %.3g, of diag(E) (dv) %.3g; max B / max|L| %.3g" % (name, sB, sE, sD, rel))
    assert sB <= 1.0 and sE <= 1.0 and sD <= 1.0
    assert rel < 1e-12


def test_reference_layout_and_small_sets():
    th = MR.data("benign", 40, 5, 11)
    ref = MR.reference(th)
    cov = np.cov(th.T, ddof=1)
    cov[np.diag_indices(5)] *= 2
    assert np.allclose(ref["Lgsl"][np.triu_indices(5, 1)], cov[np.triu_indices(5, 1)], rtol=1e-10)
    assert np.allclose(ref["L"] @ ref["L"].T, cov, rtol=1e-9)
    assert np.allclose(ref["dv"], np.diag(cov), rtol=1e-12)
    assert np.all(MR.reference(th[:1], factor=False)["dv"] == 0.0)
    assert np.all(MR.cov_bound(th[:1]) == 0.0) and np.all(MR.dv_bound_two_pass(th[:1]) == 0.0)
    # the column-wise copies of the reference and of E's diagonal agree with the matrix forms
    for t in (th, MR.data("far", 300, 7, 12), MR.data("sorted", 257, 3, 13), th[:1]):
        assert np.allclose(MR.dv_ld(t).astype(np.float64), np.diag(MR.cov_ld(t)).astype(np.float64), rtol=1e-15, atol=0)
        assert np.allclose(MR.dv_bound_gram(t), np.diag(MR.cov_bound(t)), rtol=1e-12, atol=0)


@pytest.mark.parametrize("variant,case", [
    ("unshifted", "benign-300x16"),            # means at 100 sd
    ("n", "benign-300x16"),
    ("undoubled", "benign-300x16"),
    ("transposed", "benign-300x16"),
    ("n", "tiny-3x2"),
    ("undoubled", "tiny-2x1"),
    ("pilot-last", "sorted-600x32"),           # the bounds are built from the true pilot; see _sorted
])
def test_wrong_variant_outside_the_bounds(variant, case):
    kw = {"unshifted": dict(shifted=False), "n": dict(nm1=False), "undoubled": dict(doubled=False),
          "transposed": dict(transposed=True), "pilot-last": dict(pilot_last=True)}[variant]
    sB, sE, sD, _ = _shares(CASES[case](), **kw)
    print("%s on %s: share of B %.3g, of E (upper) %.3g, of diag(E) (dv) %.3g" % (variant, case, sB, sE, sD))
    assert max(sB, sE, sD) > 1.0


def test_unshifted_at_ten_sd_is_what_a_loose_bound_hides():
    """the collinear case's means are 10 sd out: the unshifted sums' error there is reported, not asserted (it sits near the bound);
    at 100 sd (above) it is far outside"""
    th = _collinear(300, 8, 3)
    print("unshifted, means at 10 sd: shares %s" % (_shares(th, shifted=False)[:3],))
    far = _shares(MR.data("benign", 300, 16, 1), shifted=False)
    print("unshifted, means at 100 sd: shares %s" % (far[:3],))
    assert max(far[:3]) > 1.0


def test_two_pass_emulation_inside_its_bound():
    for kind, K, P, seed in [("benign", 300, 5, 21), ("far", 1000, 4, 22), ("sorted", 257, 3, 23), ("benign", 2, 2, 24), ("far", 3, 2, 25)]:
        th = MR.data(kind, K, P, seed)
        ref = MR.reference(th, factor=False)
        dv = np.array([MR.emulate_two_pass_dv(th[:, p]) for p in range(P)])
        s = MR.share(np.abs(dv.astype(MR.LD) - np.diag(ref["cov"])).astype(np.float64), MR.dv_bound_two_pass(th))
        print("two-pass %s %dx%d: share of E2 %.3g" % (kind, K, P, s))
        assert s <= 1.0
    assert MR.emulate_two_pass_dv(np.array([4.2])) == 0.0


def test_two_pass_constant_column():
    """the kernel as it was (mean of the raw values) against the kernel centred on the first row, on constant columns: the first
    is reported -- non-zero wherever the block sum / K misses the constant --, the second is exactly 0.0"""
    seen = 0
    for c in (0.1, 1.0 / 3.0, 7.3, 1e-3):
        for K in (100, 300, 4097):
            col = np.full(K, c)
            old = MR.emulate_two_pass_dv(col, centre_first_row=False)
            new = MR.emulate_two_pass_dv(col)
            print("constant %r, K = %d: dv %.3g with the raw mean, %r centred on the first row" % (c, K, old, new))
            seen += old > 0.0
            assert new == 0.0
            assert MR.emulate(np.column_stack([col, np.arange(K, dtype=np.float64)]))["dv"][0] == 0.0      # the Gram path
    assert seen > 0
