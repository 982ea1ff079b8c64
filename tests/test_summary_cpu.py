"""The NumPy reference of the weighted posterior quantiles and CDF (tests/_summary_ref.py) against hand-computed cases,
NumPy's "hazen" quantiles and its own consistency.  No GPU."""
import numpy as np
import pytest

import _summary_ref as R


def test_hand_cases_equal_weights():
    v = np.array([3.0, 1.0, 2.0, 4.0])            # sorted 1 2 3 4, knots (r + 0.5) / 4 = 0.125 0.375 0.625 0.875
    q, _ = R.summary(v, probs=(0.0, 0.125, 0.25, 0.5, 0.875, 0.9, 1.0))
    assert q.tolist() == [1.0, 1.0, 1.5, 2.5, 4.0, 4.0, 4.0]   # clamped at both ends; the median of 4 is the midpoint


def test_single_value_and_repeated_unsorted_levels():
    q, cdf = R.summary([7.5], probs=(0.9, 0.1, 0.5, 0.9), truth=7.5)
    assert q.tolist() == [7.5] * 4 and cdf == 0.5
    q, _ = R.summary([5.0, 1.0, 3.0], probs=(0.5, 0.0, 0.5, 1.0))
    assert q.tolist() == [3.0, 1.0, 3.0, 5.0]


def test_ties_signed_zeros_and_zero_weights():
    u, om = R.sorted_segment([0.0, -0.0, 1.0, -0.0], [1.0, 2.0, 0.0, 3.0])
    assert [np.signbit(x) for x in u] == [True, True, False] and om.tolist() == [2.0, 3.0, 1.0]   # -0 first, ties by e
    q, cdf = R.summary([2.0, 2.0, 1.0, 9.0], [1.0, 1.0, 1.0, 0.0], probs=(0.5,), truth=2.0)
    assert q.tolist() == [2.0] and cdf == pytest.approx((1 + 0.5 * 2) / 3, abs=0)
    _, cdf = R.summary([0.0, 1.0], truth=-0.0)           # -0 == +0: half weight
    assert cdf == 0.25
    _, cdf = R.summary([0.0, 1.0], truth=np.inf)
    assert cdf == 1.0
    _, cdf = R.summary([0.0, 1.0], truth=-np.inf)
    assert cdf == 0.0
    _, cdf = R.summary([0.0, 1.0], truth=np.nan)
    assert np.isnan(cdf)


def test_weighted_hand_case():
    # om 1 3 at u 0 10: W 1 4, knots (1 - 0.5) / 4 = 0.125, (4 - 1.5) / 4 = 0.625
    q, cdf = R.summary([10.0, 0.0], [3.0, 1.0], probs=(0.125, 0.375, 0.625), truth=10.0)
    assert q.tolist() == [0.0, 5.0, 10.0] and cdf == (1 + 1.5) / 4


def test_nonfinite_value_gives_nan():
    q, cdf = R.summary([1.0, np.inf, 2.0], truth=1.0)
    assert np.isnan(q).all() and np.isnan(cdf)


@pytest.mark.parametrize("n", [1, 2, 3, 10, 101, 1000])
def test_hazen_within_two_ulp_of_range(n):
    rng = np.random.default_rng(n)
    v = rng.normal(size=n) * 3 + 1
    probs = np.concatenate([[0.0, 1.0, 0.5], rng.uniform(size=20)])
    q, _ = R.summary(v, probs=probs)
    ref = np.quantile(v, probs, method="hazen")
    span = np.ptp(v) if n > 1 else 1.0
    assert np.all(np.abs(q - ref) <= 2 * np.spacing(span))


def test_monotone_in_q_and_cdf_inverts_quantile():
    rng = np.random.default_rng(3)
    v = rng.normal(size=5000)
    w = rng.uniform(0.1, 1.0, size=5000)
    probs = np.linspace(0.0, 1.0, 64)
    q, _ = R.summary(v, w, probs=probs)
    assert np.all(np.diff(q) >= 0)
    u, om = R.sorted_segment(v, w)
    _, W = R.knots(om)
    for p, x in zip(probs[5:-5], q[5:-5]):
        assert abs(R.cdf_sorted(u, om, W, x) - p) < 2e-3      # F(Q(q)) ~ q on continuous data (one knot spacing)


def test_long_double_reference_agrees_with_float64():
    rng = np.random.default_rng(4)
    v = rng.normal(size=777)
    w = rng.uniform(0.0, 1.0, size=777)
    for q in (0.025, 0.3, 0.5, 0.975):
        q64, _ = R.summary(v, w, probs=(q,))
        q0, tol = R.quantile_bound(v, w, q, v.size)
        assert abs(q64[0] - q0) <= tol
