"""Every projection kernel and dispatch branch (abcsmc_amd/csrc/project.hip, mirrored by tests/_project_dispatch.py) against the
oracle's projection, bit for bit, on FABRICATED model records: the test chooses M, A, the component count model[0], the
zero-variance metrics and the magnitudes, and no model fit is on the path.

The kernels promise one operation order -- the m-ascending fma chain of true-division z-scores, the k-ascending fma chain of
squared differences, sqrt -- so every comparison is np.array_equal on the uint64 views.  (The one exception: the classes of
non-finite rows, test_non_finite_rows.)  On a handful of rows the oracle itself is held to exact-rational fma chains
(fractions.Fraction), and the device with it, whatever machine compiled the oracle.

Per case: X goes in with a leading dimension beyond n (the gap rows NaN), dist sits inside a NaN-filled buffer at a chosen
8-byte offset with guard words on both sides, and the case asserts through the mirror the kernels it means to reach before it
runs.  test_cases_reach_every_kernel_and_branch holds the union of those plans to everything the mirror can reach."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _pls_ref as PR
from _project_dispatch import NOT_A_SHAPE, fused_plan, plan, reachable
from test_gpu_stats import _dev_cols

pytestmark = pytest.mark.gpu

GUARD = 4                       # NaN words on either side of dist
SPOT_ROWS = (0, 1, 63, 64, 255, 256, -2, -1)
SPOT_CHEAP = 256                # M x ncomp up to which every case checks all its spot rows


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- fabricated records ------------------------------------------------------------------------------------------------
def _fabricate(n, M, P, A, ncomp, seed, simple=False, zv=None):
    """rows X (n x M) and a model record for (M, P, A) with the header k_pls_fit writes, (ncomp, A, n, 0):
      * mean and sd on per-metric scales over 1e-3..1e3; the metrics zv (default: one or two of them once M >= 2) have sd exactly 0
        while their X values vary, so a kernel that does not skip them shows;
      * R with entries over about sixteen decades, every column's largest near 1 on a live metric;
      * observed scores (all A of them: a kernel that takes more than model[0] shows) that are the scores of a point of the cloud,
        so that the distances do not collapse onto one term;
      * everything the projection does not read (Q, W, P, H, PRESS, per) NaN."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 3, M + P)
    mean = scale * rng.normal(size=M + P)
    sdn = scale * rng.uniform(0.5, 2.0, M + P)
    if zv is None:
        zv = ([M // 2] if M >= 2 else []) + ([M - 1] if M >= 6 else [])
    sd = sdn.copy()
    sd[list(zv)] = 0.0
    live = [m for m in range(M) if m not in zv]
    X = np.asfortranarray(mean[:M] + sdn[:M] * rng.normal(size=(n, M)))
    Am = max(A, 1)
    R = rng.normal(size=(M, Am)) * 10.0 ** -rng.uniform(0, 16, (M, Am))
    for k in range(Am):
        if live:
            R[live[k % len(live)], k] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
    R = np.asfortranarray(R)
    zo = rng.normal(size=M)
    zo[list(zv)] = 0.0
    osc = zo @ R
    o = PR.model_layout(M, P, 0 if simple else A)
    m = np.full(o["len"], np.nan)
    m[0:4] = (0.0, 0.0, n, 0.0) if simple else (ncomp, A, n, 0.0)
    m[o["mean"]:o["mean"] + M + P] = mean
    m[o["sd"]:o["sd"] + M + P] = sd
    m[o["zobs"]:o["zobs"] + M] = zo
    if not simple:
        m[o["oscore"]:o["oscore"] + A] = osc[:A]
        m[o["R"]:o["R"] + M * A] = R[:, :A].reshape(-1, order="F")
    return {"X": X, "mean": mean[:M].copy(), "sd": sd[:M].copy(), "sdn": sdn[:M].copy(), "R": R[:, :A] if A else R[:, :0],
            "oscore": osc[:A], "zobs": zo, "model": m, "zv": list(zv), "live": live}


def _reference(oracle, rec, X, ncomp, simple):
    M = X.shape[1]
    if simple:          # the same chains: s_k = fma(z_k, 1, 0) = z_k (every other term adds an exact 0), then k ascending
        return oracle.project_distance(X, rec["mean"], rec["sd"], np.eye(M), M, rec["zobs"])
    return oracle.project_distance(X, rec["mean"], rec["sd"], rec["R"], ncomp, rec["oscore"][:ncomp])


def _exact_row(rec, x, ncomp, simple):
    """one row's distance with every fma evaluated exactly (one rounding each)"""
    mean, sd = rec["mean"], rec["sd"]
    z = [0.0 if sd[m] == 0.0 else float((np.float64(x[m]) - mean[m]) / sd[m]) for m in range(len(x))]
    if simple:
        t = [float(np.float64(z[m]) - rec["zobs"][m]) for m in range(len(x))]
    else:
        t = [float(np.float64(PR.fma_dot(z, rec["R"][:, k])) - rec["oscore"][k]) for k in range(ncomp)]
    d2 = 0.0
    for v in t:
        d2 = float(Fraction(v) * Fraction(v) + Fraction(d2))
    return math.sqrt(d2)


def _spot_rows(n, M, ncomp, spot):
    rows = sorted({r if r >= 0 else n + r for r in SPOT_ROWS if -n <= r < n})
    if M * max(ncomp, 1) <= SPOT_CHEAP:
        return rows
    if spot:            # wide records: the first and the last two rows, and 64 where it exists
        return sorted({r for r in rows if r in (0, 1, 64, n - 2, n - 1)})
    return []


def _project(gpu_ctx, rec, X, ld, xoff, doff, M, P, A, simple, want):
    """abc_project_distance_dev on X with leading dimension ld, xoff doubles off its allocation, dist doff doubles off a 16-byte
    boundary; want: (main, tail, second) the call must reach by the mirror -> the n distances"""
    import torch
    from abcsmc_amd import _lib
    lib = _lib.lib()
    n = X.shape[0]
    assert PR.model_layout(M, P, 0 if simple else A)["len"] == lib.abc_model_len(M, P, 0 if simple else A)
    tX, pX = _dev_cols(X, ld, xoff)
    buf = torch.full((GUARD + doff + n + GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    pD = buf.data_ptr() + 8 * (GUARD + doff)
    assert buf.data_ptr() % 16 == 0 and (tX.data_ptr() % 16 == 0)
    p = plan(n, ld, pX % 16 == 0, pD % 16 == 0, M, A, simple)
    assert (p["main"], p["tail"], p["second"]) == tuple(want), "the case does not reach what it means to: %s" % (p,)
    model = torch.from_numpy(rec["model"]).to("cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.check(lib.abc_project_distance_dev(gpu_ctx.handle, pX, n, ld, M, P, A, model.data_ptr(), int(simple), pD))
    torch.cuda.synchronize()
    d = buf.cpu().numpy()
    assert np.isnan(d[:GUARD + doff]).all() and np.isnan(d[GUARD + doff + n:]).all(), "distances written outside [0, n)"
    assert np.array_equal(_bits(model.cpu().numpy()), _bits(rec["model"])), "the model record was written to"
    return d[GUARD + doff:GUARD + doff + n].copy()


# ---- the cases ---------------------------------------------------------------------------------------------------------
# (n, M, A, ncomp, odd_ld, xoff, doff, simple, zv, spot, (main, tail, second))
CASES = []


def _add(n, M, A, ncomp, main, tail=None, second=False, odd_ld=False, xoff=0, doff=0, simple=False, zv=None, spot=False):
    CASES.append((n, M, A, ncomp, odd_ld, xoff, doff, simple, zv, spot, (main, tail, second)))


def _kc(A):
    return 1 if A <= 1 else 2 if A <= 2 else 4 if A <= 4 else 8 if A <= 8 else 16 if A <= 16 else 32


def _pair_kernel(M, A):
    """the row-pair kernel of (M, A) for A <= 32 (a restatement for the tables; _project holds it to the mirror)"""
    kc = _kc(A)
    if kc == 32:
        return ("mfma", 2, "stage" if M <= 248 else "loadings") if M <= 560 else ("dist2", 32)
    if kc in (8, 16) and (M + 1) * kc * 8 <= 65536:
        return ("dist2_lds", kc)
    return ("dist2", kc)


def _pairs(n, M, A, ncomp, **kw):
    _add(n, M, A, ncomp, _pair_kernel(M, A), ("dist", _kc(A)) if n & 1 else None, **kw)


def _build_cases():
    # every pair-kernel width with its tail: dist2<1, 2, 4>, dist2_lds<8, 16>; the LDS kernel's pipeline is written out in chunks
    # of four and eight metrics and clamps its loads at M - 1
    for A in (1, 2, 3, 4, 5, 8, 9, 16):
        for i, M in enumerate((1, 3, 4, 5, 7, 8, 9, 13)):
            for j, n in enumerate((2, 3, 257, 1000, 1001)):
                _pairs(n, M, A, (A, max(A - 1, 1), (A + 1) // 2)[(i + j) % 3])
    # the same with pairs switched off, each condition of vec_ok in turn: k_project_dist<KC> alone, KC 1..32
    for A in (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 32):
        for M in (3, 9):
            only = ("dist", _kc(A))
            _add(259, M, A, A, None, only, odd_ld=True)
            _add(260, M, A, max(A - 2, 1), None, only, xoff=1)
            _add(259, M, A, (A + 1) // 2, None, only, doff=1)
            _add(1, M, A, A, None, only)
    # the LDS kernel at exactly 65536 bytes, and one metric more: the scalar-operand kernels dist2<16>, dist2<8>
    for M, A, nc in ((511, 16, 16), (511, 9, 5), (1023, 8, 8), (1023, 5, 3), (512, 16, 16), (512, 11, 11), (1024, 8, 8), (1024, 6, 2)):
        _pairs(600, M, A, nc, spot=True)
        _pairs(601, M, A, nc)
    # the matrix pipe: steps below, at and above PF = 8 (M <= 28, 29..32, more), M mod 4 in 0..3, every n class (a lone pair,
    # one wave full and not, several work-groups, an odd last row), the component counts that leave the second tile empty
    ncs = lambda A: (A, 16, 17, 3, 0)
    for a, A in enumerate((17, 24, 32)):
        for i, M in enumerate((5, 28, 29, 37, 64)):
            for j, n in enumerate((2, 64, 66, 130, 1001, 2502)):
                _pairs(n, M, A, ncs(A)[(a + i + j) % 5])
        for nc in ncs(A):
            _pairs(130, 37, A, nc, spot=nc == A)
            _pairs(1001, 30, A, nc)
        # the two layouts (the observed scores behind the stage, behind the loadings), the upper edge, and past it: dist2<32>
        for i, M in enumerate((248, 249, 252, 560, 561)):
            _pairs(130, M, A, ncs(A)[(a + i) % 5], spot=(A == 32))
            _pairs(1001, M, A, ncs(A)[(a + i + 2) % 5])
    _pairs(200, 561, 32, 32, spot=True)
    _pairs(300, 37, 20, 13, spot=True)
    # more than 32 components: two, three and four chunks, A > M, aligned and 8 bytes off
    # (component counts: all, 40 -- 32 under A = 33: the second chunk all zero --, none)
    for A in (33, 64, 65, 96, 97):
        for i, nc in enumerate((A, min(40, A - 1), 0)):
            for M in (2, 50):
                for xoff in (0, 1):
                    _add(300 + (M == 2) + 2 * xoff, M, A, nc, ("wide", (A + 31) // 32 * 32), xoff=xoff, odd_ld=(i == 1), spot=(i == 0))
    _add(100, 5, 70, 65, ("wide", 96), spot=True)
    # the simple distance, with a zero-variance metric (M = 1: with and without)
    for M in (1, 7, 48):
        for n in (1, 2, 257, 1001):
            for xoff in (0, 1):
                _add(n, M, 0, 0, ("simple",), simple=True, xoff=xoff, doff=xoff ^ (n & 1), odd_ld=bool(n & 1), spot=True)
    _add(257, 1, 0, 0, ("simple",), simple=True, zv=[0])
    # no component at all: every distance is +0.0
    for A, M in ((3, 5), (8, 6), (12, 7)):
        _pairs(259, M, A, 0)
        _add(259, M, A, 0, None, ("dist", _kc(A)), xoff=1)
    # nothing padded: ncomp = A = KC in the scalar-operand, the LDS and the one-row kernels
    for A in (1, 2, 4, 8, 16, 32):
        _pairs(515, 11, A, A)
    # the second trip of every grid-stride loop: three work-groups and one row past the clamp
    _add(2097152 + 769, 2, 2, 2, ("dist2", 2), ("dist", 2), second=True, spot=True)
    _add(524288 + 770, 4, 8, 6, ("dist2_lds", 8), None, second=True, spot=True)
    _add(1048576 + 769, 2, 3, 3, None, ("dist", 4), second=True, xoff=1, spot=True)
    _add(1048576 + 769, 2, 0, 0, ("simple",), None, second=True, simple=True, spot=True)
    _add(1048576 + 769, 2, 33, 20, ("wide", 64), None, second=True, spot=True)


_build_cases()


def _id(c):
    n, M, A, ncomp, odd_ld, xoff, doff, simple, zv, spot, want = c
    kern = want[0] or want[1]
    return "%s-n%d-M%d-A%d-nc%d%s%s%s%s" % ("_".join(str(v) for v in kern), n, M, A, ncomp, "-oddld" if odd_ld else "",
                                           "-xoff" if xoff else "", "-doff" if doff else "", "-zv" if zv else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_project_distance_bit_exact(gpu_ctx, oracle, case):
    n, M, A, ncomp, odd_ld, xoff, doff, simple, zv, spot, want = case
    P = 3 if M % 2 else 7
    big = n > 100000
    rec = _fabricate(n, M, P, A, ncomp, seed=1000003 * M + 1009 * A + 31 * ncomp + n % 977, simple=simple, zv=zv)
    X = rec["X"]
    even = n + 2 + (n & 1)
    ld = even + 1 if odd_ld else even
    ref = _reference(oracle, rec, X, ncomp, simple)
    rows = _spot_rows(n, M, ncomp, spot)
    if big:
        rows = [0, n - 1]
    for r in rows:
        ex = _exact_row(rec, X[r], ncomp, simple)
        assert _bits(ref[r]) == _bits(ex), "the oracle differs from the exact fma chains at row %d: %r %r" % (r, ref[r], ex)
    if not simple and ncomp == 0:
        assert not _bits(ref).any(), "no component: every distance is +0.0"
    elif rec["live"]:
        assert np.isfinite(ref).all() and len(np.unique(ref)) > min(n, 3) // 2, "degenerate reference distances"
    d = _project(gpu_ctx, rec, X, ld, xoff, doff, M, P, A, simple, want)
    bad = np.flatnonzero(_bits(d) != _bits(ref))
    assert bad.size == 0, "%d of %d distances differ from the oracle, first at row %d: %r, oracle %r" % (
        bad.size, n, bad[0], d[bad[0]], ref[bad[0]])


def test_cases_reach_every_kernel_and_branch():
    """through the mirror of launch_project_distance: the union of the plans the cases assert is everything it can reach --
    every dist2 width, dist2_lds<8, 16>, both layouts of the matrix-pipe kernel, the wide kernel on two to four chunks, the
    simple kernel, every dist<KC> as a tail and as the only kernel -- and the second trip of all five grid-stride loops"""
    wants = [c[-1] for c in CASES]
    mains, tails, only = reachable()
    assert {w[0] for w in wants if w[0] is not None} == mains
    assert {w[1] for w in wants if w[0] is not None and w[1] is not None} == tails
    assert {w[1] for w in wants if w[0] is None} == only
    assert mains >= {("dist2", kc) for kc in (1, 2, 4, 8, 16, 32)} | {("dist2_lds", 8), ("dist2_lds", 16), ("mfma", 2, "stage"),
                                                                     ("mfma", 2, "loadings"), ("wide", 64), ("wide", 96), ("simple",)}
    assert tails == only == {("dist", kc) for kc in (1, 2, 4, 8, 16, 32)}
    assert {w[0] or w[1] for w in wants if w[2]} == {("dist2", 2), ("dist2_lds", 8), ("dist", 4), ("simple",), ("wide", 64)}
    # the component counts: none, fewer than 17 under 32 (the second matrix tile all zero), all of them with nothing padded
    fam = lambda c: (c[-1][0] or c[-1][1])[0]
    assert {fam(c) for c in CASES if not c[7] and c[3] == 0} == {"dist2", "dist2_lds", "mfma", "wide", "dist"}
    assert {c[3] for c in CASES if fam(c) == "mfma"} >= {0, 3, 16, 17, 24, 32}
    assert {c[2] for c in CASES if c[2] == c[3] and c[2] == _kc(c[2])} == {1, 2, 4, 8, 16, 32}
    # the dynamic LDS at both limits
    assert {(M, A) for n, M, A, *_ in CASES if plan(n, n + 2, True, True, M, A, False)["lds"] == 65536} >= {(511, 16), (1023, 8)}
    assert any(plan(c[0], c[0] + 2, True, True, c[1], c[2], False)["lds"] == 152576 for c in CASES if not c[7])


# ---- the fused pass of the batched rankings -------------------------------------------------------------------------------
# (N, M, A, ncomp, kernel of launch_project_distance_scores)
FUSED = [(N, M, A, nc, kern)
         for M, A, kern in ((13, 8, ("dist2_lds", 8)), (21, 12, ("dist2_lds", 16)), (37, 24, ("mfma", 2, "stage")))
         for N in (2000, 2002) for nc in (A, 3)]
FUSED += [(2000, M, A, nc, NOT_A_SHAPE) for M, A in ((512, 16), (561, 24)) for nc in (A, 3)]


@pytest.mark.parametrize("case", FUSED, ids=lambda c: "N%d-M%d-A%d-nc%d" % c[:4])
def test_rank_targets_on_fabricated_records(gpu_ctx, oracle, case):
    """device.rank_targets with K = N on a fabricated record: the scores of every row come from launch_project_distance_scores
    (Sout and dist set, row_split = 0, nc_force = A, model[0] = A or 3) or, where that is not a shape for it, from the batched
    path's own kernel; per target the whole ranking -- indices and distances -- equals the oracle's projection and order"""
    import torch
    from abcsmc_amd import device
    N, M, A, ncomp, kern = case
    P, B = 3, 3
    rec = _fabricate(N, M, P, A, ncomp, seed=77 * M + A + ncomp + N)
    X = rec["X"]
    dX = device.colmajor(X, "cuda:0")
    dY = torch.zeros((P, N), dtype=torch.float64, device="cuda:0")
    assert dX.data_ptr() % 16 == 0 and dX.stride(0) == N
    # (dist and S come from the library's arena, on 256-byte boundaries)
    assert fused_plan(N, N, True, M, A, 0, N) == kern
    rng = np.random.default_rng(5 + M)
    T = np.empty((B, M))
    T[0] = X[17]                                                        # a row of X: distance 0
    T[1] = rec["mean"] + rec["sdn"] * rng.normal(size=M)                # inside the cloud
    T[2] = rec["mean"] + 1e3 * rec["sdn"] * rng.choice([-1.0, 1.0], M)  # far outside
    dT = torch.from_numpy(np.ascontiguousarray(T.T)).to("cuda:0")       # (M, B) holder
    model = torch.from_numpy(rec["model"]).to("cuda:0")
    idx, dist, _ = device.rank_targets(dX, model, A, dT, N, Y=dY, ctx=gpu_ctx)
    torch.cuda.synchronize()
    idx, dist = idx.cpu().numpy().astype(np.uint64), dist.cpu().numpy()
    for b in range(B):
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(rec["sd"] == 0, 0.0, (T[b] - rec["mean"]) / rec["sd"])
        o = np.array([PR.fma_dot(z, rec["R"][:, k]) for k in range(ncomp)])
        d = oracle.project_distance(X, rec["mean"], rec["sd"], rec["R"], ncomp, o)
        order = oracle.ordered(d)
        if b == 0:
            assert d[17] == 0.0 and order[0] == 17 and np.count_nonzero(d == 0.0) == 1
        assert np.array_equal(idx[b], order), "target %d: %d ranks differ" % (b, int(np.sum(idx[b] != order)))
        assert np.array_equal(_bits(dist[b]), _bits(d[order.astype(np.int64)])), "target %d: distances differ in bits" % b


# ---- non-finite rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,A,ncomp,simple,main", [(5, 3, 2, False, ("dist2", 4)), (9, 6, 5, False, ("dist2_lds", 8)),
                                                   (21, 20, 18, False, ("mfma", 2, "stage")), (7, 40, 35, False, ("wide", 64)),
                                                   (7, 0, 0, True, ("simple",))])
def test_non_finite_rows(gpu_ctx, oracle, M, A, ncomp, simple, main):
    """NaN in a live metric gives NaN; NaN or inf in a zero-variance metric gives the finite reference value (bit for bit); +inf
    in a live metric gives +inf in the reference and, in a kernel that pads its components (ncomp < KC: fma(inf, 0, s) = NaN),
    NaN -- DESIGN.md, declared deviations: both sort behind every finite distance.  So: the finite rows equal the reference in
    bits, the non-finite rows are the reference's, and NaN stays NaN."""
    n, P = 400, 3
    rec = _fabricate(n, M, P, A, ncomp, seed=4242 + M)
    X = rec["X"].copy(order="F")
    live, zv = rec["live"][0], rec["zv"][0]
    nan_live, nan_zv, inf_zv, inf_live = (3, 130), (4, 131), (64, 257), (65, 399)
    X[list(nan_live), live] = np.nan
    X[list(nan_zv), zv] = np.nan
    X[inf_zv[0], zv], X[inf_zv[1], zv] = np.inf, -np.inf
    X[list(inf_live), rec["live"][-1]] = np.inf
    if simple:          # (the identity loadings of _reference would turn the infinite z-score into fma(inf, 0, s) = NaN)
        with np.errstate(divide="ignore", invalid="ignore"):
            Z = np.where(rec["sd"] == 0, 0.0, (X - rec["mean"]) / rec["sd"])
        ref = np.sqrt(((Z - rec["zobs"]) ** 2).sum(1))
        clean = np.isfinite(ref)
        ref[clean] = _reference(oracle, rec, np.asfortranarray(X[clean]), ncomp, True)
    else:
        ref = _reference(oracle, rec, X, ncomp, False)
    assert np.isnan(ref[list(nan_live)]).all() and np.isposinf(ref[list(inf_live)]).all()
    assert np.isfinite(ref[list(nan_zv + inf_zv)]).all() and np.isfinite(ref).sum() == n - 4
    d = _project(gpu_ctx, rec, X, n + 2, 0, 0, M, P, A, simple, (main, None, False))
    assert np.array_equal(np.isfinite(d), np.isfinite(ref)), np.flatnonzero(np.isfinite(d) != np.isfinite(ref))
    assert np.isnan(d[np.isnan(ref)]).all()
    fin = np.isfinite(ref)
    assert np.array_equal(_bits(d[fin]), _bits(ref[fin]))
