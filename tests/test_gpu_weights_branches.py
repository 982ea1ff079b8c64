"""Every kernel branch of the weight stage (abcsmc_amd/csrc/weights.hip) against tests/_weights_ref.py, the long-double
statement of ABC::weight_predictive_prior: the edges of the split-operand kernel's exact range from both sides, the far-row
fix-ups at every width and variant, the fp64 stand-in behind the split kernel at every width and for every reason, row
sub-ranges, small and ragged sets, the Epanechnikov instances.  tests/_weights_dispatch.py says which kernels a case runs and
which kernel word (abc_kde_last_kernel) it must leave; test_cases_reach_every_instance holds the cases against everything the
launchers can reach.

Tolerances, relative, per raw weight (the project's own figures, tests/test_gpu_parity.py: KDE_TOL and the comment above it):
    rows summed in fp64 (far new rows, every row of a stand-in or fp64 call)      1e-9
    rows of the split kernel: its stated budget       5e-7 up to 16 parameters, 5.5e-7 at 17..32, 8e-7 at 33..64
Every case asserts: the kernel word the mirror predicts, weights of 0 exactly where the reference has them (nowhere, but for
the Epanechnikov rows without support), a repeated call bit-identical.

Measured on an MI355X, worst error per variant over all cases of this file (`pytest -s` prints every case and, at the end, this
table); the file's 149 tests take 20 s:
    split rows   k_kde_split<1>      1.51e-7   <KS_FOLD + 1>      1.58e-7   <KS_TOPN + 1>      9.23e-8     (budget 5e-7)
                 k_kde_split<2>      9.26e-8   <KS_FOLD + 2>      2.21e-7   <KS_TOPN + 2>      1.08e-7     (5.5e-7)
                 k_kde_split_lds<3>  3.28e-7   <KS_FOLD + 3>      2.31e-7   <KS_TOPN + 3>      2.40e-7     (8e-7)
                 k_kde_split_lds<4>  1.30e-7   <KS_FOLD + 4>      4.70e-7   <KS_TOPN + 4>      1.87e-7     (8e-7)
                 (the largest, 4.70e-7 at 61 parameters, in the shifted range of test_whole_range_shifted_to_its_edges)
    fp64 rows    far new rows behind the split kernels  9.4e-13       the stand-in, k_kde_fixups<8 .. 64>   8.2e-13
                 k_kde<2 .. 64>  8.1e-13       k_kde_gen  7.8e-13       k_epan<2 .. 64>, k_kde_gen's Epanechnikov branch  7.6e-15
"""
import numpy as np
import pytest

import _weights_dispatch as D
import _weights_ref as R
from test_gpu_parity import KDE_TOL, _weights_case

pytestmark = pytest.mark.gpu

GAUSS, UNIF_INT = R.PRIOR_GAUSS, R.PRIOR_UNIF_INT
K0, KP0 = 300, 700          # ten column slices, 22 previous tiles (the last one partial), two row blocks of the pair kernels
FP64, SPLIT = D.RAN_FP64, D.RAN_SPLIT

def _budget(P):
    """the split kernel's error budget for a weight that one term dominates (tests/test_gpu_parity.py, above KDE_TOL)"""
    return 5e-7 if P <= 16 else 5.5e-7 if P <= 32 else 8e-7


# ---- the cases, as (P, kn, K', kde mode, weight kernel, top-order variant forced): what the mirror needs to say which kernels run
P_ALL = [5, 8, 9, 13, 14, 16, 17, 29, 30, 32, 33, 45, 46, 48, 49, 61, 62, 64]
P_FULL = [14, 16, 30, 32, 46, 48, 62, 64]                      # full chunks: the top-order variant exists
P_STANDIN = [7, 12, 16, 24, 32, 40, 64]
REASONS = ["converged", "beyond", "far_new", "far_prev"]
RANGES = [(0, 300), (1, 255), (44, 256), (43, 257)]
P_RANGES = [13, 16, 40, 49, 64]
KP_EDGES = [1, 31, 32, 33, 63, 64, 65]
K_EDGES = [1, 255, 256, 257]
P_EPAN = [2, 3, 6, 12, 20, 40]
P_FP64 = [2, 3, 7, 12, 20, 40]


def _declared():
    c = set()
    c |= {(P, K0, KP0, "auto", "gauss", False) for P in P_ALL} | {(P, K0, 2049, "auto", "gauss", True) for P in P_FULL}
    c |= {(P, K0, Kp, "auto", "gauss", False) for P in (12, 16) for Kp in (KP0, 1300)}                      # (b)
    c |= {(P, K0, KP0, "auto", "gauss", False) for P in (13, 16, 29, 48, 61)}                                # (c)
    c |= {(P, K0, Kp, "auto", "gauss", False) for P in P_STANDIN for Kp in (KP0, 1300)}                      # (d)
    c |= {(P, K0, KP0, "auto", "gauss", False) for P in (70, 130)}
    c |= {(P, 150, KP0, "auto", "gauss", False) for P in P_STANDIN + [70, 130]}
    c |= {(P, kn, KP0, "auto", "gauss", False) for P in P_RANGES for _, kn in RANGES}                        # (e)
    c |= {(P, K0, Kp, "auto", "gauss", False) for P in (12, 16, 40) for Kp in KP_EDGES}                      # (f)
    c |= {(P, K, KP0, "auto", "gauss", False) for P in (12, 16) for K in K_EDGES}
    c |= {(16, K0, Kp, "auto", "gauss", True) for Kp in (2047, 2048, 2049)}
    c |= {(P, K0, KP0, "auto", "epan", False) for P in P_EPAN} | {(100, 150, KP0, "auto", "epan", False)}    # (g)
    c |= {(P, K0, KP0, "fp64", "gauss", False) for P in P_FP64}                                              # (h)
    return c


DECLARED = _declared()
WORST = {}


@pytest.fixture(autouse=True)
def _defaults(gpu_ctx, monkeypatch):
    """the library's default weight kernels before and after every test; the top-order variant only where a case forces it"""
    from abcsmc_amd import _lib
    monkeypatch.delenv("ABC_KDE_TOPN_MIN_PAIRS", raising=False)
    yield
    gpu_ctx.set_kde_mode(_lib.KDE_AUTO)
    gpu_ctx.set_weight_kernel(_lib.WEIGHT_GAUSSIAN)


def _flat(P):
    """flat priors: their 64-fold product stays a normal number, and no moved row leaves the support"""
    return [(GAUSS, 0.0, 1e4)] * P


def _base(P, K=K0, Kp=KP0, seed=0, binades=0):
    """_weights_case's sets; K' rows of a previous set of at least 700 (its doubled variance is the whole set's, so that a set
    of one row has one); binades: previous weights spread over that many"""
    wl, th, tp, wp, dv = _weights_case(P, K, max(Kp, KP0), 9000 + 13 * P + seed)
    th, tp, wp = th.copy(), tp[:Kp].copy(), wp[:Kp].copy()
    if binades:
        wp *= np.exp2(np.random.default_rng(3 + P).uniform(-binades, 0, Kp))
    return wl, th, tp, wp, dv.copy()


def _unit(dv):
    """one scaled unit of every parameter (k_wprep: the rows are scaled by sqrt(log2 e) / sqrt(dv))"""
    return np.sqrt(np.where(dv != 0, dv, 1.0)) / D.SQRT_LOG2E


def _direction(rng, P, norm2, n=None, cmax=7.5):
    """rows of squared norm norm2 with every coordinate taking part: magnitudes within 0.6 .. 1 of one another, or as close to one
    another as it takes to keep every coordinate below cmax"""
    lo = max(0.6, np.sqrt(norm2 / P) / cmax)
    assert lo < 1.0
    v = rng.uniform(lo, 1.0, (n or 1, P)) * rng.choice([-1.0, 1.0], (n or 1, P))
    v *= np.sqrt(norm2 / (v * v).sum(axis=1))[:, None]
    return v if n else v[0]


def _gpu_raw(gpu_ctx, spec, th, tp, wp, dv, k0, kn):
    """abc_weights_raw_dev twice -> (weights, weights again, the two kernel words)"""
    import torch
    from abcsmc_amd import _lib, device, sharded
    dev = "cuda:0"
    be = sharded.HipBackend(dev, gpu_ctx)
    dth, dtp, dwp, ddv = (device.colmajor(np.asfortranarray(a), dev) for a in (th, tp, wp, dv))
    dpri = device.priors_to_device(_lib.make_priors(spec), dev)
    out, words = [], []
    for _ in range(2):
        o = torch.full((kn,), -1.0, dtype=torch.float64, device=dev)
        be.weights_raw(dpri, dth, k0, kn, dtp, dwp, ddv, o)
        torch.cuda.synchronize()
        words.append(gpu_ctx.kde_last_kernel())
        out.append(o.cpu().numpy())
    return out[0], out[1], words


def _check(gpu_ctx, tag, spec, th, tp, wp, dv, k0=0, kn=None, mode="auto", epan=False, topn=False, expect=None,
           monkeypatch=None, normalised=False):
    """one case through abc_weights_raw_dev (and abc_weight_predictive_prior: normalised) against the reference; -> (w, ref)"""
    from abcsmc_amd import _lib, abcutil
    K, P = th.shape
    Kp = tp.shape[0]
    kn = K - k0 if kn is None else kn
    rows = slice(k0, k0 + kn)
    assert (P, kn, Kp, mode, "epan" if epan else "gauss", topn) in DECLARED, "a case the table at the top does not declare"
    pl = D.plan(P, kn, Kp, mode, "epan" if epan else "gauss", 0.0 if topn else D.TOPN_MIN_PAIRS)
    word = D.ran(pl, th[rows], tp, wp, dv)
    assert expect is None or word == expect, "the case is not what it was built to be: the mirror predicts %d" % word
    assert pl["topn"] == topn
    if epan:
        ref = R.epanechnikov(spec, th[rows], tp, wp, dv, normalise=False)
    else:
        ref = R.raw(spec, th[rows], tp, wp, dv)
        assert np.all(np.isfinite(ref)) and np.all(ref > 0), "the case drops a row"
    ref = ref.astype(np.float64)
    assert np.all(np.isfinite(ref)) and np.all((ref == 0) | (ref > 1e-300))
    gpu_ctx.set_kde_mode(_lib.KDE_FP64 if mode == "fp64" else _lib.KDE_AUTO)
    gpu_ctx.set_weight_kernel(_lib.WEIGHT_EPANECHNIKOV if epan else _lib.WEIGHT_GAUSSIAN)
    if topn:
        monkeypatch.setenv("ABC_KDE_TOPN_MIN_PAIRS", "0")
    w, w2, words = _gpu_raw(gpu_ctx, spec, th, tp, wp, dv, k0, kn)
    assert words == [word, word], "kernel word %s, the mirror predicts %d" % (words, word)
    assert np.array_equal(w, w2), "a repeated call differs"
    assert np.array_equal(w == 0, ref == 0)
    ok = ref > 0
    err = np.zeros(kn)
    err[ok] = np.abs(w[ok] - ref[ok]) / ref[ok]
    # which rows were summed in fp64: all of them unless the split kernel ran, then the far new rows (k_kde_fixups)
    in_fp64 = D.far(th[rows], tp, wp, dv)[0] if word == SPLIT else np.ones(kn, dtype=bool)
    e64 = float(err[in_fp64].max()) if in_fp64.any() else 0.0
    esp = float(err[~in_fp64].max()) if (~in_fp64).any() else 0.0
    key = pl["pair"] if word == SPLIT else ("standin", pl["fixup"]) if pl["split"] else pl["pair"]
    WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0, 0.0)), (esp, e64)))
    print("%s P = %d rows [%d, %d) of %d, K' = %d: %s word %d, split rows %.2e (%d), fp64 rows %.2e (%d)" %
          (tag, P, k0, k0 + kn, K, Kp, key, word, esp, (~in_fp64).sum(), e64, in_fp64.sum()))
    assert e64 < KDE_TOL["fp64"], (tag, P, e64)
    assert esp < _budget(P), (tag, P, esp)
    if normalised:
        # the whole call as the drop-in makes it: the same raw weights (the same launcher on the same rows), divided by their
        # L2 norm -- summed in another order than here, hence 1e-12
        assert k0 == 0 and kn == K
        wn = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp, wp, dv, ctx=gpu_ctx)
        assert gpu_ctx.kde_last_kernel() == word
        wl = w.astype(np.longdouble)
        assert np.max(np.abs(wn - (wl / np.sqrt((wl * wl).sum())).astype(float)) / wn) < 1e-12
        assert np.linalg.norm(wn) == pytest.approx(1.0, rel=1e-12)
    return w, ref


# ---- (a) every pair kernel with far rows on both sides ---------------------------------------------------------------------
def _far_both_sides(P, Kp=KP0, binades=0, new_rows=(3, 20, 43), extra_new=()):
    """previous weights of 0; one new and one previous row far by one coordinate; one of each far by the norm alone (from seven
    parameters on); one previous row far by its weight on each side (2^-301; 2^101, far enough out for the others' terms to
    count beside its own); a far new row whose nearest previous row is far too; extra_new: more far new rows"""
    wl, th, tp, wp, dv = _base(P, K0, Kp, binades=binades)
    rng = np.random.default_rng(100 + P)
    unit, c = _unit(dv), D.centre(tp, dv)
    wp[1::97] = 0.0
    i_coord, i_norm, i_pair = new_rows
    far_i, far_j = [i_coord, i_pair], [10, 60, 61, 90]
    th[i_coord, 2 % P] = c[2 % P] + 11.0 * unit[2 % P]
    tp[10, P - 1] = c[P - 1] - 10.5 * unit[P - 1]
    if P >= 7:
        n2 = 415.0 if P < 10 else 440.0                                 # (seven parameters: 400 / 7 is 7.56 squared already)
        th[i_norm] = c + _direction(rng, P, n2, cmax=7.85) * unit
        tp[50] = c + _direction(rng, P, n2, cmax=7.85) * unit
        far_i.append(i_norm)
        far_j.append(50)
    wp[60] = 2.0 ** -301
    wp[61] = 2.0 ** 101
    tp[61] = c
    tp[61, :4] = c[:4] + 7.25 * unit[:4] * np.array([1.0, -1.0, 1.0, -1.0])        # 14.5 units out, squared norm 210: far by weight only
    d = rng.normal(size=P)
    d *= 12.0 / np.abs(d).max()
    th[i_pair] = c + d * unit
    tp[90] = th[i_pair] + 0.2 * unit * rng.normal(size=P)
    for n, i in enumerate(extra_new):
        th[i, (5 + n) % P] = c[(5 + n) % P] - (9.0 + n) * unit[(5 + n) % P]
        far_i.append(i)
    fi, fj, beyond = D.far(th, tp, wp, dv)
    assert sorted(np.flatnonzero(fi)) == sorted(far_i) and sorted(np.flatnonzero(fj)) == sorted(far_j) and not beyond
    if P >= 7:      # by the norm alone
        a, b = (th[i_norm] - D.centre(tp, dv)) * D.scale(dv), (tp[50] - D.centre(tp, dv)) * D.scale(dv)
        assert np.abs(a).max() < 8.0 and np.abs(b).max() < 8.0 and (a * a).sum() > 400 and (b * b).sum() > 400
    return th, tp, wp, dv


@pytest.mark.parametrize("P", P_ALL)
def test_every_pair_kernel_with_far_rows_on_both_sides(gpu_ctx, P):
    th, tp, wp, dv = _far_both_sides(P)
    _check(gpu_ctx, "(a)", _flat(P), th, tp, wp, dv, expect=SPLIT, normalised=True)


@pytest.mark.parametrize("P", P_FULL)
def test_top_order_variants_with_far_rows_on_both_sides(gpu_ctx, monkeypatch, P):
    """tiles in the order of the rows' norm tops (forced at a test's size), previous weights over 60 binades: the sparse ends of
    the order make wide tiles, handled the plain way inside the same kernel"""
    th, tp, wp, dv = _far_both_sides(P, Kp=2049, binades=60)
    _check(gpu_ctx, "(a) top order", _flat(P), th, tp, wp, dv, topn=True, expect=SPLIT, monkeypatch=monkeypatch)


@pytest.mark.parametrize("P", [5, 8])
def test_far_in_one_coordinate_whichever_at_two_lanes_per_row(gpu_ctx, P):
    """k_wrows<1> below nine parameters: two lanes per row, the second one without a parameter of its own but with the row's norm
    pieces (the folded variant), so it has to learn that the row is far.  The far previous row carries a weight 2^36 times the
    others': what the split kernel would add for it, were its norm pieces not blanked, is then as large as the ordinary terms"""
    wl, th0, tp0, wp0, dv = _base(P, seed=1)
    unit, c = _unit(dv), D.centre(tp0, dv)
    for idx in range(P):
        th, tp, wp = th0.copy(), tp0.copy(), wp0.copy()
        j, q = (7 * idx + 5) % KP0, P - 1 - idx
        th[3 + idx, idx] = c[idx] + 11.0 * unit[idx]
        tp[j, q] = c[q] - 8.5 * unit[q]
        wp[j] *= 2.0 ** 36
        fi, fj, _ = D.far(th, tp, wp, dv)
        assert list(np.flatnonzero(fi)) == [3 + idx] and list(np.flatnonzero(fj)) == [j]
        _check(gpu_ctx, "(a) coordinate %d" % idx, _flat(P), th, tp, wp, dv, expect=SPLIT)


# ---- (b) the bounds from both sides, observed through the kernel word ------------------------------------------------------
def _edge_rows(P, n_out, n_in, kind):
    """n_out new rows just outside the exact range and n_in just inside: one coordinate at 8.1 / 7.9 units (kind "coordinate"), or
    a squared norm of 405 / 395 with every coordinate below 7.5 ("norm")"""
    wl, th, tp, wp, dv = _base(P, seed=2)
    rng = np.random.default_rng(200 + P)
    unit, c = _unit(dv), D.centre(tp, dv)
    out, ins = np.arange(n_out) * 3 % K0, 200 + np.arange(n_in)          # (n_out <= 100: distinct rows below 300; the others from 200 on)
    assert len(set(out) | set(ins)) == n_out + n_in
    for rows, coord, norm2 in ((out, 8.1, 405.0), (ins, 7.9, 395.0)):
        for n, i in enumerate(rows):
            if kind == "coordinate":
                th[i, n % P] = c[n % P] + (coord if n & 1 else -coord) * unit[n % P]
            else:
                v = _direction(rng, P, norm2)
                assert np.abs(v).max() < 7.5
                th[i] = c + v * unit
    fi, fj, beyond = D.far(th, tp, wp, dv)
    assert sorted(np.flatnonzero(fi)) == sorted(out) and not fj.any() and not beyond
    return th, tp, wp, dv


@pytest.mark.parametrize("kind", ["coordinate", "norm"])
@pytest.mark.parametrize("P", [12, 16])
def test_range_edges_of_the_new_rows(gpu_ctx, P, kind):
    """rows inside a bound are not counted, rows outside are: with L = kn / 16 + 32 rows just outside (and 40 just inside) the call
    stays on the split kernel, with L + 1 the fp64 stand-in takes it; with none outside, the rows just inside keep the budget"""
    L = K0 // 16 + 32
    assert L == D.plan(P, K0, KP0)["lim_i"] == 50
    _check(gpu_ctx, "(b) %s, all inside" % kind, _flat(P), *_edge_rows(P, 0, 40, kind), expect=SPLIT)
    _check(gpu_ctx, "(b) %s, L outside" % kind, _flat(P), *_edge_rows(P, L, 40, kind), expect=SPLIT)
    _check(gpu_ctx, "(b) %s, L + 1 outside" % kind, _flat(P), *_edge_rows(P, L + 1, 40, kind), expect=FP64)


@pytest.mark.parametrize("side", ["low", "high"])
@pytest.mark.parametrize("P", [12, 16])
def test_range_edges_of_the_previous_weights(gpu_ctx, P, side):
    """1024 previous rows of weight 2^-301 (2^101) are far, 100 of 2^-299 (2^99) are not: split kernel and column fix-up; one far
    row more and the fp64 stand-in takes the call"""
    outside, inside = (2.0 ** -301, 2.0 ** -299) if side == "low" else (2.0 ** 101, 2.0 ** 99)
    for n_far, expect in ((0, SPLIT), (D.KS_MAX_FAR_J, SPLIT), (D.KS_MAX_FAR_J + 1, FP64)):
        wl, th, tp, wp, dv = _base(P, Kp=1300, seed=3)
        order = np.random.default_rng(300 + P).permutation(1300)
        wp[order[:n_far]] = outside
        wp[order[n_far:n_far + 100]] = inside
        fi, fj, _ = D.far(th, tp, wp, dv)
        assert fj.sum() == n_far and not fi.any()
        _check(gpu_ctx, "(b) weights %s, %d far" % (side, n_far), _flat(P), th, tp, wp, dv, expect=expect)


# ---- (c) the whole range shifted -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(281, 299), (-99, -81)])
@pytest.mark.parametrize("P", [13, 16, 29, 48, 61])
def test_whole_range_shifted_to_its_edges(gpu_ctx, P, lo, hi):
    """previous weights all within [2^-299, 2^-281] (within [2^81, 2^99]) and every new row beside a previous one at a squared
    norm of about 395, whose term dominates the row's sum: the exact part of the split kernel's exponent has no slack left, and
    nothing is far"""
    wl, th, tp, wp, dv = _base(P, seed=4)
    rng = np.random.default_rng(400 + P + lo)
    unit = _unit(dv)
    wp = np.exp2(-rng.uniform(lo, hi, KP0))
    # 150 pairs of previous rows at +d and -d around the centre of the rows that stay: the centre (the first row plus the mean
    # clipped offset) does not move, so the norms are what they are built to be
    moved = np.arange(100, 400)
    stay = np.ones(KP0, dtype=bool)
    stay[moved] = False
    c = D.centre(tp[stay], dv)
    d = _direction(rng, P, 1.0, 150) * np.sqrt(rng.uniform(0.97, 1.0, 150) * 395.0)[:, None]
    tp[moved[:150]] = c + d * unit
    tp[moved[150:]] = c - d * unit
    assert np.max(np.abs(D.centre(tp, dv) - c) / unit) < 1e-9
    a = (tp[moved] - c) / unit + 0.15 * rng.normal(size=(300, P))       # new row i beside previous row 100 + i ...
    a *= np.sqrt(rng.uniform(0.97, 1.0, 300) * 395.0 / (a * a).sum(axis=1))[:, None]        # ... at a squared norm of 383 .. 395 itself
    th[:] = c + a * unit
    fi, fj, beyond = D.far(th, tp, wp, dv)
    assert not fi.any() and not fj.any() and not beyond
    b = (tp - c) * D.scale(dv)
    assert np.abs(a).max() < 7.5 and ((b[moved] ** 2).sum(axis=1) > 383).all()
    # the neighbour's term dominates: more than 0.99 of the row's sum
    ld = R.log_denominator(th, tp, wp, dv)
    own = R.log_denominator(th[:1], tp[100:101], wp[100:101], dv)
    assert float(np.exp(own[0] - ld[0])) > 0.99
    _check(gpu_ctx, "(c) weights 2^-[%d, %d]" % (lo, hi), _flat(P), th, tp, wp, dv, expect=SPLIT)


# ---- (d) the fp64 stand-in behind the split kernel, at every width and for every reason -------------------------------------
def _declined(P, reason):
    Kp = 1300 if reason == "far_prev" else KP0
    wl, th, tp, wp, dv = _base(P, Kp=Kp, seed=5)
    rng = np.random.default_rng(500 + P)
    unit, c = _unit(dv), D.centre(tp, dv)
    spec = _flat(P) if P <= 64 else wl.prior_spec()
    if reason == "converged":
        # dv' = 0 in parameter 2; both sets take two values there, rows in no order: factor 1 where they agree, 0 where not
        dv[2] = 0.0
        th[:, 2] = np.where(rng.random(K0) < 0.5, 7.0, 8.0)
        tp[:, 2] = np.where(rng.random(Kp) < 0.25, 8.0, 7.0)
        spec = list(spec)
        spec[2] = (UNIF_INT, 1, 10)
    elif reason == "beyond":
        tp[17, 1] = c[1] + 3000.0 * unit[1]              # exponents may leave int32: the guarded fp64 loop (its term is exactly 0)
        assert D.far(th, tp, wp, dv)[2]
    elif reason == "far_new":
        lim = K0 // 16 + 32
        for n in range(lim + 1):
            th[5 * n, n % P] = c[n % P] + 11.0 * unit[n % P]
        assert D.far(th, tp, wp, dv)[0].sum() == lim + 1
    else:
        wp[rng.permutation(Kp)[:D.KS_MAX_FAR_J + 1]] = 2.0 ** -301
        assert D.far(th, tp, wp, dv)[1].sum() == D.KS_MAX_FAR_J + 1
    return spec, th, tp, wp, dv


@pytest.mark.parametrize("reason", REASONS)
@pytest.mark.parametrize("P", P_STANDIN)
def test_stand_in_at_every_width(gpu_ctx, P, reason):
    """kde_body behind k_kde_fixups<8 | 16 | 32 | 64>: the split kernel is launched and declines"""
    spec, th, tp, wp, dv = _declined(P, reason)
    assert D.plan(P, K0, tp.shape[0])["split"]
    _check(gpu_ctx, "(d) %s" % reason, spec, th, tp, wp, dv, expect=FP64)


@pytest.mark.parametrize("P", P_STANDIN + [70, 130])
def test_converged_parameter_in_a_row_sub_range(gpu_ctx, P):
    """the converged-parameter rule reads the raw rows k0 + i of the new set (the sharded driver's call): rows 37 .. 186 of 300;
    beyond 64 parameters k_kde_gen, the whole set and the sub-range"""
    spec, th, tp, wp, dv = _declined(P, "converged")
    assert (th[37:187, 2] != th[:150, 2]).sum() > 40                   # (row i and row k0 + i differ: a dropped k0 shows)
    _check(gpu_ctx, "(d) converged, k0 = 37", spec, th, tp, wp, dv, k0=37, kn=150, expect=FP64)
    if P > 64:
        _check(gpu_ctx, "(d) converged", spec, th, tp, wp, dv, expect=FP64)


# ---- (e) row sub-ranges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0,kn", RANGES)
@pytest.mark.parametrize("P", P_RANGES)
def test_row_sub_ranges_with_far_rows(gpu_ctx, P, k0, kn):
    """abc_weights_raw_dev on rows k0 .. k0 + kn - 1 of 300: far new rows inside and outside the range (0, 3, 20, 43, 299), far
    previous rows; against the reference's rows"""
    th, tp, wp, dv = _far_both_sides(P, extra_new=(0, 299))
    _check(gpu_ctx, "(e)", _flat(P), th, tp, wp, dv, k0=k0, kn=kn, expect=SPLIT)


# ---- (f) small and ragged sets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kp", KP_EDGES)
@pytest.mark.parametrize("P", [12, 16, 40])
def test_small_previous_sets(gpu_ctx, P, Kp):
    """one previous row, and either side of a 32-row tile and of the 64 rows per slice (40 parameters: tiles staged in LDS)"""
    wl, th, tp, wp, dv = _base(P, Kp=Kp, seed=6)
    wp[1::5] = 0.0
    _check(gpu_ctx, "(f) K' = %d" % Kp, _flat(P), th, tp, wp, dv, expect=SPLIT)


@pytest.mark.parametrize("K", K_EDGES)
@pytest.mark.parametrize("P", [12, 16])
def test_small_and_ragged_new_sets(gpu_ctx, P, K):
    """one new row, and either side of the 256 rows of a work-group"""
    wl, th, tp, wp, dv = _base(P, K=K, seed=7)
    wp[1::5] = 0.0
    _check(gpu_ctx, "(f) K = %d" % K, _flat(P), th, tp, wp, dv, expect=SPLIT)


@pytest.mark.parametrize("Kp", [2047, 2048, 2049])
def test_top_order_variant_around_the_rank_kernels_chunk(gpu_ctx, monkeypatch, Kp):
    """the ranks by norm top are counted in chunks of 2048 rows (k_wq_hist, k_wq_rank): one chunk short of a row, full, and a second
    chunk of one row"""
    wl, th, tp, wp, dv = _base(16, Kp=Kp, seed=8, binades=60)
    wp[1::101] = 0.0
    _check(gpu_ctx, "(f) top order, K' = %d" % Kp, _flat(16), th, tp, wp, dv, topn=True, expect=SPLIT, monkeypatch=monkeypatch)


# ---- (g) Epanechnikov ------------------------------------------------------------------------------------------------------
def _epan_case(P, K=K0):
    wl, th, tp, wp, dv = _base(P, K=K, seed=9)
    if P > 4:
        dv[2] = 0.0                                                      # a converged parameter takes no part
    return wl.prior_spec(), th, tp, wp, dv


@pytest.mark.parametrize("P", P_EPAN)
def test_epanechnikov_at_every_width(gpu_ctx, P):
    """k_epan<2 .. 64> with the checks of test_weight_epanechnikov_extension: a row nothing supports gets weight 0, the others match
    to 1e-9, zeros where the reference has them, L2 norm 1"""
    from abcsmc_amd import _lib, abcutil
    spec, th, tp, wp, dv = _epan_case(P)
    th[5] = th[5] + 40 * np.sqrt(np.where(dv > 0, dv, 1.0))              # far from everything: no support
    assert D.plan(P, K0, KP0, weight_kernel="epan")["pair"] == ("epan", D.padded_width(P))
    w, ref = _check(gpu_ctx, "(g)", spec, th, tp, wp, dv, epan=True, expect=FP64)
    assert w[5] == 0.0 and ref[5] == 0.0 and (ref > 0).sum() > K0 // 2
    gpu_ctx.set_weight_kernel(_lib.WEIGHT_EPANECHNIKOV)
    wn = abcutil.weight_predictive_prior(_lib.make_priors(spec), th, tp, wp, dv, ctx=gpu_ctx)
    refn = R.epanechnikov(spec, th, tp, wp, dv)
    ok = refn > 0
    assert np.allclose(wn[ok], refn[ok], rtol=1e-9, atol=0) and np.array_equal(wn == 0, refn == 0)
    assert np.linalg.norm(wn) == pytest.approx(1.0, rel=1e-12)


def test_epanechnikov_beyond_64_parameters_in_a_row_sub_range(gpu_ctx):
    """k_kde_gen's Epanechnikov branch with a converged parameter, rows 37 .. 186 of 300"""
    spec, th, tp, wp, dv = _epan_case(100)
    th[37 + 5] = th[37 + 5] + 40 * np.sqrt(np.where(dv > 0, dv, 1.0))
    assert D.plan(100, 150, KP0, weight_kernel="epan")["pair"] == ("gen", True)
    w, ref = _check(gpu_ctx, "(g)", spec, th, tp, wp, dv, k0=37, kn=150, epan=True, expect=FP64)
    assert w[5] == 0.0 and ref[5] == 0.0 and (ref > 0).sum() > 75


# ---- (h) fp64 on request: k_kde<2 .. 64> -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", P_FP64)
def test_fp64_kernel_at_every_width(gpu_ctx, P):
    """the fp64 kernel of its own launch (ABC_KDE_FP64, and below five parameters), far rows on both sides: nothing is far for it"""
    if P >= 5:
        th, tp, wp, dv = _far_both_sides(P)
    else:
        wl, th, tp, wp, dv = _base(P)
        unit, c = _unit(dv), D.centre(tp, dv)
        th[3, 0] = c[0] + 11.0 * unit[0]
        tp[10, P - 1] = c[P - 1] - 10.5 * unit[P - 1]
        wp[1::97] = 0.0
    assert D.plan(P, K0, KP0, kde_mode="fp64")["pair"] == ("kde", D.padded_width(P))
    _check(gpu_ctx, "(h)", _flat(P), th, tp, wp, dv, mode="fp64", expect=FP64)


# ---- the cases against everything the launchers can reach ------------------------------------------------------------------
def test_cases_reach_every_instance():
    """through the mirror: the declared cases (every _check asserts that it is one of them) reach every pair kernel, every k_wrows
    instance and every fix-up width the launchers can reach -- the fix-ups both for far rows and as the stand-in"""
    pairs, wrows, fix = set(), set(), set()
    for P, kn, Kp, mode, wk, topn in DECLARED:
        pl = D.plan(P, kn, Kp, mode, wk, 0.0 if topn else D.TOPN_MIN_PAIRS)
        pairs.add(pl["pair"])
        wrows.add(pl["wrows"])
        fix.add(pl["fixup"])
    r_pairs, r_wrows, r_fix = D.reachable()
    assert pairs == r_pairs, sorted(r_pairs - pairs)
    assert wrows - {None} == r_wrows and fix - {None} == r_fix
    # far rows at every fix-up width (a), the stand-in at every width (d)
    assert {D.padded_width(P) for P in P_ALL} == r_fix == {D.padded_width(P) for P in P_STANDIN}
    assert {D.plan(P, K0, KP0)["pair"] for P in P_ALL} | {D.plan(P, K0, 2049, topn_min_pairs=0.0)["pair"] for P in P_FULL} == \
        {k for k in r_pairs if k[0].startswith("split")}
    # (after the cases, in file order: what they measured)
    for key in sorted(WORST, key=str):
        print("worst of %-22s split rows %.2e, fp64 rows %.2e" % ((str(key),) + WORST[key]))
