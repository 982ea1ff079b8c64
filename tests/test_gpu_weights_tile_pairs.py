"""The pair sums of the one-chunk families with TWO tiles per batch (abcsmc_amd/csrc/weights.hip: kz_pair_sums, the instance
k_kde_split<.., TPB 2> of the folded and the top-order family; the plain family keeps the one-tile loop) against
tests/_weights_ref.py, the long-double statement of ABC::weight_predictive_prior, at the smallest shapes at which the new loop
can go wrong: slices of one, two, three and four tiles and of both parities, a ragged last tile, one and two row blocks, a wide
tile as the first and as the second of a pair, two tiles of a pair more than 126 binades apart, a tile of zero-weight rows
beside an ordinary one, far rows on both sides inside one pair.

Tolerance: the kernels' stated budget, 5e-7 relative per non-zero raw weight up to 16 parameters (1e-9 for the rows the fp64
fix-ups sum), an identical zero pattern, a repeated call bit-identical.

Largest relative error per family in this file, measured on an MI355X (`pytest -s` prints every case), beside the figures
of tests/test_gpu_weights_branches.py for the one-tile loop:
    k_kde_split<1>            (one tile per batch)     this file 1.75e-7     branches 1.51e-7
    k_kde_split<KS_FOLD + 1>  (two tiles per batch)    this file 2.03e-7     branches 1.58e-7 (one tile per batch)
    k_kde_split<KS_TOPN + 1>  (two tiles per batch)    this file 2.07e-7     branches 9.23e-8 (one tile per batch)
(the branch tests themselves pass unchanged on the two-tile kernels).  The file's 68 tests take 3 s.
"""
import numpy as np
import pytest

import _weights_dispatch as D
import _weights_ref as R
from test_gpu_parity import KDE_TOL
from test_gpu_weights_branches import _base, _flat, _gpu_raw, _unit

pytestmark = pytest.mark.gpu

BUDGET = 5e-7                                   # up to 16 parameters
FAMILIES = [(5, False), (13, False), (14, False), (16, False), (14, True), (16, True)]      # (P, top order forced)
KP_EDGES = [32, 33, 64, 65, 96, 97, 160]
K_EDGES = [1, 255, 256, 257]
WORST = {}


@pytest.fixture(autouse=True)
def _defaults(gpu_ctx, monkeypatch):
    from abcsmc_amd import _lib
    monkeypatch.delenv("ABC_KDE_TOPN_MIN_PAIRS", raising=False)
    gpu_ctx.set_kde_mode(_lib.KDE_AUTO)
    gpu_ctx.set_weight_kernel(_lib.WEIGHT_GAUSSIAN)
    yield


def _slice_tiles(pl):
    """the tiles of every column slice, as the kernels cut them: [nbt sl / slices, nbt (sl + 1) / slices)"""
    nbt, s = pl["tiles"], pl["slices"]
    return [nbt * (i + 1) // s - nbt * i // s for i in range(s)]


def _check(gpu_ctx, monkeypatch, tag, th, tp, wp, dv, topn, ref=None):
    K, P = th.shape
    Kp = tp.shape[0]
    pl = D.plan(P, K, Kp, "auto", "gauss", 0.0 if topn else D.TOPN_MIN_PAIRS)
    assert pl["chunks"] == 1 and pl["split"] and pl["topn"] == topn and D.ran(pl, th, tp, wp, dv) == D.RAN_SPLIT
    if ref is None:
        ref = R.raw(_flat(P), th, tp, wp, dv)
    ref = ref.astype(np.float64)
    assert np.all(np.isfinite(ref)) and np.all(ref > 0)
    if topn:
        monkeypatch.setenv("ABC_KDE_TOPN_MIN_PAIRS", "0")
    w, w2, words = _gpu_raw(gpu_ctx, _flat(P), th, tp, wp, dv, 0, K)
    assert words == [D.RAN_SPLIT, D.RAN_SPLIT]
    assert np.array_equal(w, w2), "a repeated call differs"
    assert np.array_equal(w == 0, ref == 0)
    err = np.abs(w - ref) / ref
    far_i = D.far(th, tp, wp, dv)[0]
    e64 = float(err[far_i].max()) if far_i.any() else 0.0
    esp = float(err[~far_i].max()) if (~far_i).any() else 0.0
    WORST[pl["pair"]] = max(WORST.get(pl["pair"], 0.0), esp)
    print("%s P = %d K = %d K' = %d %s slices %s: split rows %.2e, fp64 rows %.2e; worst so far %s" %
          (tag, P, K, Kp, pl["pair"], _slice_tiles(pl), esp, e64, {k: "%.2e" % v for k, v in WORST.items()}))
    assert e64 < KDE_TOL["fp64"], (tag, e64)
    assert esp < BUDGET, (tag, esp)
    return w


def test_the_shapes_cut_slices_of_both_parities():
    """what the shapes below are chosen for: slices of one tile, of two, three and four (whole pairs with and without a one-tile
    batch behind them), and -- K' = 160, the smallest that the small-set rule s <= K' / 64 lets have two slices -- two slices of
    different parity in one launch"""
    seen = set()
    for P, topn in FAMILIES:
        for Kp in KP_EDGES:
            for K in K_EDGES:
                pl = D.plan(P, K, Kp, "auto", "gauss", 0.0 if topn else D.TOPN_MIN_PAIRS)
                assert pl["pair"] == ("split", 1 + (D.KS_TOPN if topn else D.KS_FOLD if P <= 13 else 0), 3)
                tiles = _slice_tiles(pl)
                assert sum(tiles) == (Kp + 31) // 32
                seen |= set(tiles)
                if Kp == 160:
                    assert tiles == [2, 3]
    assert seen == {1, 2, 3, 4}


@pytest.mark.parametrize("Kp", KP_EDGES)
@pytest.mark.parametrize("P,topn", FAMILIES)
def test_every_slice_shape_and_row_block_count(gpu_ctx, monkeypatch, P, topn, Kp):
    """previous weights over 40 binades (the batch references of neighbouring tiles then differ); the reference once for the 257
    rows, the calls on their first 1, 255, 256 and 257"""
    wl, th, tp, wp, dv = _base(P, 257, Kp, seed=5, binades=40)
    ref = R.raw(_flat(P), th, tp, wp, dv)
    for K in K_EDGES:
        _check(gpu_ctx, monkeypatch, "shapes", th[:K].copy(), tp, wp, dv, topn, ref[:K])


def _hb(tp, wp, dv):
    b = (tp - D.centre(tp, dv)) * D.scale(dv)
    return 0.5 * (b * b).sum(axis=1) - np.log2(wp)


@pytest.mark.parametrize("wide_first", [True, False])
@pytest.mark.parametrize("P", [14, 16])
def test_top_order_one_wide_tile_in_a_pair(gpu_ctx, monkeypatch, P, wide_first):
    """64 previous rows = one pair of tiles in the order of the tops hb = 1/2|b|^2 - log2 w': 32 rows with their tops within 0.02
    of one another (a narrow tile) and 32 spread over 25 units below them (the wide tile comes first) or above them (second)"""
    wl, th, tp, wp, dv = _base(P, 257, 64, seed=6)
    rng = np.random.default_rng(60 + P)
    delta = np.concatenate([rng.uniform(-0.01, 0.01, 32), (-1.0 if wide_first else 1.0) * np.linspace(5.0, 30.0, 32)])
    delta = delta[rng.permutation(64)]
    b = (tp - D.centre(tp, dv)) * D.scale(dv)
    wp = np.exp2(0.5 * (b * b).sum(axis=1) - (40.0 + delta))
    hb = np.sort(_hb(tp, wp, dv))
    spread = [hb[:32].max() - hb[:32].min(), hb[32:].max() - hb[32:].min()]
    assert (spread[0] > 20 and spread[1] < 0.1) if wide_first else (spread[0] < 0.1 and spread[1] > 20)
    assert abs(hb[32] - hb[31]) > 4.0                      # the two groups are the two tiles, however ties inside one are ordered
    for K in (1, 257):
        _check(gpu_ctx, monkeypatch, "one wide tile (%s)" % ("first" if wide_first else "second"), th[:K].copy(), tp, wp, dv, True)


@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("P,topn", FAMILIES)
def test_tiles_of_a_pair_more_than_126_binades_apart(gpu_ctx, monkeypatch, P, topn, lower):
    """the weights of one tile of the pair 2^-250 times the other's: for EVERY new row the largest exponent of the lower tile lies
    more than 126 below that of the other, so under the pair's one reference every term of the lower tile flushes to zero; they
    are below 2^-126 of the row's sum, which the reference keeps"""
    wl, th, tp, wp, dv = _base(P, 257, 64, seed=7)
    low = np.arange(32 * lower, 32 * lower + 32)
    high = np.arange(32 * (1 - lower), 32 * (1 - lower) + 32)
    wp[low] *= 2.0 ** -250
    assert not D.far(th, tp, wp, dv)[1].any()
    c, sc = D.centre(tp, dv), D.scale(dv)
    E = ((th - c) * sc) @ ((tp - c) * sc).T - _hb(tp, wp, dv)[None, :]            # a term's base-2 exponent, up to the row's factor
    assert (E[:, high].max(axis=1) - E[:, low].max(axis=1)).min() > 126
    assert _hb(tp, wp, dv)[low].min() - _hb(tp, wp, dv)[high].max() > 126          # (top order: the two groups are the two tiles)
    _check(gpu_ctx, monkeypatch, "126 binades", th, tp, wp, dv, topn)


@pytest.mark.parametrize("P,topn", FAMILIES)
def test_zero_weight_tile_and_far_rows_inside_one_pair(gpu_ctx, monkeypatch, P, topn):
    """96 previous rows = a pair and a one-tile batch; rows 32..63 have weight 0 (a tile of hb = KS_HB_ZERO rows: the second of the
    pair, or with the tiles in top order the last); far previous rows in both ordinary tiles, a far new row among ordinary ones in
    each row block"""
    wl, th, tp, wp, dv = _base(P, 257, 96, seed=8)
    unit, c = _unit(dv), D.centre(tp, dv)
    wp[32:64] = 0.0
    tp[10, P - 1] = c[P - 1] - 10.5 * unit[P - 1]
    tp[70, 0] = c[0] + 9.5 * unit[0]
    th[3, 2] = c[2] + 11.0 * unit[2]
    th[256, 1] = c[1] - 9.0 * unit[1]
    fi, fj, beyond = D.far(th, tp, wp, dv)
    assert list(np.flatnonzero(fi)) == [3, 256] and list(np.flatnonzero(fj)) == [10, 70] and not beyond
    _check(gpu_ctx, monkeypatch, "zero tile, far rows", th, tp, wp, dv, topn)


@pytest.mark.parametrize("P,topn", [(13, False), (16, False), (16, True)])
def test_far_rows_in_both_tiles_of_a_pair(gpu_ctx, monkeypatch, P, topn):
    """64 previous rows, one far row in each tile of the pair (all-zero limbs and hb = KS_HB_ZERO inside otherwise ordinary tiles)"""
    wl, th, tp, wp, dv = _base(P, 255, 64, seed=9)
    unit, c = _unit(dv), D.centre(tp, dv)
    tp[5, 1] = c[1] + 8.5 * unit[1]
    tp[40, 3] = c[3] - 12.0 * unit[3]
    fi, fj, beyond = D.far(th, tp, wp, dv)
    assert not fi.any() and list(np.flatnonzero(fj)) == [5, 40] and not beyond
    _check(gpu_ctx, monkeypatch, "far in both tiles", th, tp, wp, dv, topn)
