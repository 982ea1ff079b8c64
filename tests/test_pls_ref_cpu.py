"""CPU checks of tests/_pls_ref.py, the long-double model of the PLS fit from a statistics record: against the oracle's fp64
fit and scikit-learn's rotations, statistics-form PRESS against residual sums, and hand-made cases with known answers."""
import os

import numpy as np
import pytest

import _pls_ref as R

LD = np.longdouble
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _data(N, M, P, seed, noise=0.3, k=5):
    rng = np.random.default_rng(seed)
    F = rng.normal(size=(N, k))
    X = F @ rng.normal(size=(k, M)) + noise * rng.normal(size=(N, M)) + rng.normal(size=M) * 3
    Y = F @ rng.normal(size=(k, P)) + noise * rng.normal(size=(N, P)) - 2.0
    return X, Y


@pytest.mark.parametrize("N,M,P,A,ntrain", [(400, 12, 5, 4, 250), (600, 30, 16, 8, 300), (300, 9, 1, 5, 200),
                                            (500, 20, 40, 6, 350)])
def test_fit_matches_oracle_fp64(oracle, N, M, P, A, ntrain):
    """the oracle's fp64 pls_fit on the z-scored training rows (whole-set moments) == the reference to 1e-10 per column, on
    components the reference calls well conditioned"""
    X, Y = _data(N, M, P, 1000 + M + P)
    s = R.stats_record(X, Y, ntrain)
    ref = R.reference(s, M, P, A)
    mean, sd = X.mean(0), X.std(0, ddof=1)
    ym, ysd = Y.mean(0), Y.std(0, ddof=1)
    Xz, Yz = (X[:ntrain] - mean) / sd, (Y[:ntrain] - ym) / ysd
    W, Pm, Q, Rr = oracle.pls_fit(Xz, Yz, A, 2)
    f = ref["fit"]
    well = ~ref["ill"]
    assert well[:min(A, 3)].all(), ref["fit"]["gap"]
    for a in np.nonzero(well)[0]:
        for dev, rf in ((Rr, f["R"]), (W, f["W"]), (Pm, f["Pl"]), (Q, f["Q"])):
            rf = rf[:, a].astype(np.float64)
            assert np.linalg.norm(dev[:, a] - rf) <= 1e-10 * np.linalg.norm(rf), (a, ref["fit"]["gap"][a])


@pytest.mark.parametrize("tag,A", [("a", 4), ("b", 8), ("c", 3)])
def test_rotations_match_sklearn(tag, A):
    z = np.load(os.path.join(G, "pls_sklearn.npz"))
    X, Y = z[tag + "_X"], z[tag + "_Y"]
    M, P = X.shape[1], Y.shape[1]
    ref = R.reference(R.stats_record(X, Y, X.shape[0]), M, P, A)
    Rr = ref["fit"]["R"].astype(np.float64)
    Rs = z[tag + "_rot"]
    sgn = np.sign((Rs * Rr).sum(0))
    assert np.abs(Rr / np.linalg.norm(Rr, axis=0) - sgn * Rs / np.linalg.norm(Rs, axis=0)).max() < 1e-6


def test_statistics_press_equals_residual_press():
    """PRESS from the validation statistics (YY - 2 q'c + q'Hq) == the sum of squared residuals of the z-scored validation rows,
    both in long double (integer rows and a zero shift: the fp64 record is exact)"""
    N, M, P, A, ntr = 500, 14, 6, 7, 300
    X, Y = _data(N, M, P, 7)
    X, Y = np.round(8 * X), np.round(8 * Y)
    X[:, 3] *= 1e4
    s = R.stats_record(X, Y, ntr, shift=np.zeros(M + P))
    ref = R.reference(s, M, P, A)
    z = ref["z"]
    Zr = np.concatenate([X, Y], 1).astype(LD) - s[2:2 + M + P].astype(LD)
    Zz = (Zr - z["d"]) / z["sd"]
    Xt, Yt = Zz[ntr:, :M], Zz[ntr:, M:]
    Rr, Q = ref["fit"]["R"].astype(np.float64).astype(LD), ref["fit"]["Q"].astype(np.float64).astype(LD)
    T = Xt @ Rr
    pr = ref["press"]["press"]
    for a in range(A):
        E = Yt - T[:, :a + 1] @ Q[:, :a + 1].T
        direct = np.sum(E * E, 0)
        assert np.all(np.abs(pr[a] - direct) <= 1e-15 * np.abs(direct)), a
    # and the bound is a bound of the fp64 evaluation: the same formula in fp64 lies within it
    c64 = ref["press"]["c"].astype(np.float64)
    H64 = ref["press"]["H"].astype(np.float64)
    Q64 = ref["fit"]["Q"].astype(np.float64)
    YY = z["YY"].astype(np.float64)
    for j in range(P):
        for a in range(A):
            q = Q64[j, :a + 1]
            p64 = YY[j] - 2 * (q @ c64[j, :a + 1]) + q @ H64[:a + 1, :a + 1] @ q
            assert abs(p64 - float(pr[a, j])) <= ref["press"]["bound"][a, j], (j, a)


def test_moments_f64_is_the_fp64_formula():
    X, Y = _data(300, 6, 3, 11)
    s = R.stats_record(X, Y, 200)
    mean, sd = R.moments_f64(s, 6, 3)
    z = R.zstats(s, 6, 3)
    assert np.allclose(mean, np.concatenate([X, Y], 1).mean(0), rtol=1e-13)
    assert np.allclose(sd, z["sd"].astype(np.float64), rtol=1e-14)


def test_single_response_closed_form():
    X, Y = _data(200, 8, 1, 3)
    ref = R.reference(R.stats_record(X, Y, 120), 8, 1, 3)
    z, f = ref["z"], ref["fit"]
    xy, XX = z["XY"][0][:, 0], z["XX"][0]
    w = xy / np.sqrt(xy @ xy)
    tt = w @ XX @ w
    assert np.allclose(f["W"][:, 0], w, rtol=1e-17, atol=0) and np.allclose(f["R"][:, 0], w, rtol=1e-17, atol=0)
    assert abs(f["tt"][0] - tt) <= 1e-17 * tt
    assert np.allclose(f["Pl"][:, 0], XX @ w / tt, rtol=1e-16, atol=1e-19)
    assert abs(f["Q"][0, 0] - xy @ w / tt) <= 1e-17 * abs(f["Q"][0, 0])
    assert (f["gap"] == 1).all() and not ref["ill"][0]


def test_degenerate_spectrum_is_flagged():
    """XY with orthonormal columns: XY'XY = I, every direction dominant"""
    XY0 = np.zeros((5, 2))
    XY0[0, 0] = XY0[1, 1] = 1.0
    f = R.fit(XY0, np.eye(5), 2)
    assert f["gap"][0] == 0.0
    e, ill = R.column_bounds(f, 5, 2, R.U)
    assert ill.all() and np.isinf(e).all()
    # a planted relative gap of 1e-4 is not flagged, its bound grows as 1 / gap
    XY0[1, 1] = np.sqrt(1 - 1e-4)
    f = R.fit(XY0, np.eye(5), 1)
    assert abs(f["gap"][0] - 1e-4) < 1e-12
    e2, ill2 = R.column_bounds(f, 5, 2, R.U)
    assert not ill2[0] and e2[0] >= 1e4 * (4 * 7 + 64) * R.U


def _ones_orthogonal_rows():
    """4 x 4 Hadamard rows: exactly orthogonal +-1 vectors"""
    H2 = np.array([[1, 1], [1, -1]])
    return np.kron(H2, H2)


def test_exact_tie_from_orthogonal_rows_is_flagged():
    Hd = _ones_orthogonal_rows().astype(float)
    X = np.concatenate([Hd, -Hd], 0)                  # 8 rows, mean 0, X'X = 8 I... (2 per sign)
    Y = np.concatenate([Hd[:, 1:3], -Hd[:, 1:3]], 0)  # two responses, each equal to a metric: XY'XY = c I
    s = R.stats_record(X, Y, 8)
    ref = R.reference(s, 4, 2, 2)
    assert ref["fit"]["gap"][0] < 1e-15 and ref["ill"].all()


def test_constant_dyadic_response():
    """a constant response (0.75: dyadic, so sums and squares are exact): sd 0, z 0, its Q row exactly 0, its PRESS row constant,
    per = 1"""
    X, Y = _data(300, 10, 3, 5)
    Y[:, 1] = 0.75
    s = R.stats_record(X, Y, 200)
    ref = R.reference(s, 10, 3, 4)
    assert ref["z"]["sd"][10 + 1] == 0
    assert (ref["fit"]["Q"][1] == 0).all()
    pr = ref["press"]
    assert (pr["press"][:, 1] == pr["press"][0, 1]).all() and pr["per"][1] == 1
    assert not ref["fit"]["zero"].any()


def test_all_responses_constant_gives_zero_components():
    X, _ = _data(300, 10, 3, 6)
    Y = np.full((300, 3), -1.5)
    ref = R.reference(R.stats_record(X, Y, 200), 10, 3, 4)
    f = ref["fit"]
    assert f["zero"].all() and not ref["ill"].any()
    for key in ("W", "R", "Pl", "Q"):
        assert (f[key] == 0).all()
    pr = ref["press"]
    assert (pr["press"] == 0).all() and (pr["per"] == 1).all() and pr["ncomp"] == 1 and (pr["H"] == 0).all()
    # P == 1, constant response
    ref1 = R.reference(R.stats_record(X, Y[:, :1], 200), 10, 1, 3)
    assert ref1["fit"]["zero"].all() and (ref1["press"]["press"] == 0).all()


def test_empty_validation_partition():
    X, Y = _data(300, 10, 4, 8)
    ref = R.reference(R.stats_record(X, Y, 300), 10, 4, 5)
    pr = ref["press"]
    assert (pr["press"] == 0).all() and (pr["per"] == 1).all() and pr["ncomp"] == 1
    assert not pr["ambiguous"].any()          # (equal PRESS: the strict argmin is the first, exactly)


@pytest.mark.parametrize("P", [3, 1])
def test_oracle_fit_of_zero_cross_products_gives_zero_components(oracle, P):
    """an exactly-zero X'Y (constant responses z-score to zeros; or every metric constant): the oracle's fit, both methods, the
    reference and the tests' numpy stage mirror all give finite, exactly zero components (declared deviations)"""
    import torch
    from _numpy_backend import NumpyBackend
    X, _ = _data(200, 9, P, 21)
    Xz = (X - X.mean(0)) / X.std(0, ddof=1)
    for Xin, Yin in ((Xz, np.zeros((200, P))), (np.zeros((200, 9)), np.random.default_rng(2).normal(size=(200, P)))):
        for method in (1, 2):
            for mat in oracle.pls_fit(Xin, Yin, 4, method):
                assert np.isfinite(mat).all() and (mat == 0).all(), method
    Y = np.full((200, P), 0.75)
    s = R.stats_record(X, Y, 120)
    ref = R.reference(s, 9, P, 4)
    assert ref["fit"]["zero"].all() and (ref["press"]["press"] == 0).all()
    be = NumpyBackend()
    model = torch.full((be.model_len(9, P, 4),), float("nan"), dtype=torch.float64)
    be.pls_model(torch.from_numpy(s), torch.from_numpy(X[0].copy()), 9, P, 4, 0, model)
    m = R.unpack_model(model.numpy(), 9, P, 4)
    assert (m["R"] == 0).all() and (m["Q"] == 0).all() and m["hdr"][0] == 1
