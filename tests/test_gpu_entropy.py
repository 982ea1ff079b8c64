"""Posterior entropy of the batched ranking (abc_rank_targets_entropy_dev, abc_particle_ranking_pls_targets_entropy,
abc_weighted_entropy*) against the long-double form of the header's definition (tests/_entropy_ref.py), built on the device's own
rows and adjusted values.

Every case checks knn^2 within 4 (P + 2) 2^-53 relative of the reference's rho2 (P + 1 roundings of the chain, margin 4), H within
1e-11 max(1, |H_ref|, (P / 2) max_e |log rho2_e|) and zeros exactly.  Then the invariances the header states (the same bits alone,
in a batch, on a repeat run, through the host and the device entries, with every member alone; knn under a row permutation; scale
against values divided beforehand), the edge rules, the refusals and the Python wrappers.

Sizes: 600 rows of 6 metrics, the set of tests/test_gpu_draws.py; P = 1 (generic), 2, 3, 5, 9, 16, 17 (EN_PREG = 16: the widest P
whose own values stay in registers; 17 takes the LDS instance; 3, 5 and 9 are padded to 4, 8 and 16); k = 1, 4, 8; K = k, k + 1,
63, 64, 65, 255, 256, 257 (EN_BS = EN_CH = 256: rows per tile and per staged chunk), 600, and 1000 for the generic entries (four
chunks); B = 1, 3, 17.

The worst knn^2 and H errors over the cases of this file, in units of their bounds, are printed by test_python_wrappers (run with
-s).  Measured on an MI355X over 177 targets: knn^2 0.225 of 4 (P + 2) 2^-53 rho2, H 3e-5 of its bound."""
import ctypes as C

import numpy as np
import pytest

import _entropy_ref as R
from test_gpu_draws import DEV, M, N, _fit, _reference_rows

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
MEMBERS = ("H", "knn", "zeros")
ENTRIES = {"targets_host": "abc_particle_ranking_pls_targets_entropy", "targets_dev": "abc_rank_targets_entropy_dev",
           "weighted_host": "abc_weighted_entropy", "weighted_dev": "abc_weighted_entropy_dev"}
LD = np.longdouble
WORST = {"knn": 0.0, "H": 0.0, "n": 0}      # largest errors of knn^2 and H over their bounds; targets compared


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def _strided(a, pad):
    """numpy (n, c) -> a (c, n) column-major holder that is a view of a (c, n + pad) tensor: row stride n + pad"""
    import torch
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[1], a.shape[0] + pad), np.nan, dtype=torch.float64, device=DEV)
    t[:, :a.shape[0]] = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)
    return t[:, :a.shape[0]]


def _call(ctx, entry, K, k=4, F=None, targets=None, Yd=None, V=None, w=None, scale=None, members=MEMBERS, method=0, kernel=1,
          null=False, pad=0):
    """One call of an entry straight through ctypes with exactly `members` of the descriptor's outputs non-NULL (null: a NULL
    descriptor).  targets entries: F (the fit) and targets (B, M); weighted entries: V (K, P) and w (K,) or None.  pad: the device
    entries read X, Y and V through views with that much row stride to spare.  Every output starts as NaN / all ones.
    -> (status, {member: numpy array})"""
    import torch
    from abcsmc_amd import _lib, device
    on_dev, tg = entry.endswith("_dev"), entry.startswith("targets")
    if tg:
        B, P = targets.shape[0], F["P"]
        lead = (B,)
    else:
        V = np.asfortranarray(V)
        P, lead = V.shape[1], ()
    shapes = dict(H=lead, knn=lead + (K,), zeros=lead)
    out = {}
    for m in members:
        if m == "zeros":
            out[m] = torch.full(shapes[m], -1, dtype=torch.int64, device=DEV) if on_dev else np.full(shapes[m], 2 ** 64 - 1, dtype=np.uint64)
        else:
            out[m] = torch.full(shapes[m], np.nan, dtype=torch.float64, device=DEV) if on_dev else np.full(shapes[m], np.nan)
    p = (lambda t: t.data_ptr()) if on_dev else (lambda v: v.ctypes.data)
    o = lambda m: p(out[m]) if m in out else None
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    desc = _lib.Entropy(k, None if sc is None else sc.ctypes.data, o("H"), o("knn"), o("zeros"))
    ref = None if null else C.byref(desc)
    fn = getattr(_lib.lib(), ENTRIES[entry])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if entry == "targets_host":
        T = np.asfortranarray(targets)
        rc = fn(ctx.handle, F["X"].ctypes.data, F["Y"].ctypes.data, N, M, P, T.ctypes.data, B, 0.5, 0, 0, None, K, method, kernel,
                None, None, None, ref, None)
    elif entry == "targets_dev":
        Td = device.colmajor(np.asfortranarray(targets), DEV)
        Xd = _strided(F["X"], pad) if pad else F["Xd"]
        Yd = (_strided(F["Y"], pad) if pad else F["Yd"]) if Yd is None else Yd
        rc = fn(ctx.handle, Xd.data_ptr(), Xd.stride(0), Yd.data_ptr(), Yd.stride(0), N, M, P, F["model"].data_ptr(), F["A"],
                Td.data_ptr(), B, B, None, K, method, kernel, None, None, None, ref)
    elif entry == "weighted_host":
        wa = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        rc = fn(ctx.handle, V.ctypes.data, K, P, None if wa is None else wa.ctypes.data, ref)
    else:
        Vd = _strided(V, pad) if pad else device.colmajor(V, DEV)
        wd = None if w is None else torch.tensor(np.ascontiguousarray(w, dtype=np.float64), device=DEV)
        rc = fn(ctx.handle, Vd.data_ptr(), K + pad, K, P, None if wd is None else wd.data_ptr(), ref)
    if on_dev:
        torch.cuda.synchronize()
        out = {m: v.cpu().numpy() for m, v in out.items()}
    if "zeros" in out:
        out["zeros"] = out["zeros"].astype(np.int64)
    return rc, out


def _ok(ctx, *a, **kw):
    rc, out = _call(ctx, *a, **kw)
    ctx.check(rc)
    return out


def _h_bound(ref, P):
    logs = ref["logs"][np.isfinite(ref["logs"])]
    top = float(np.abs(logs).max()) if logs.size else 0.0
    return 1e-11 * max(1.0, abs(float(ref["H"])) if np.isfinite(ref["H"]) else 0.0, 0.5 * P * top)


def _check_target(vals, out, b, k, scale=None):
    """target b of the outputs (out[name][b]; b = () for the generic entries) against the reference of its values (K, P)"""
    K, P = vals.shape
    ref = R.entropy(vals, k, scale)
    H, knn, zeros = out["H"][b], out["knn"][b], out["zeros"][b]
    assert zeros == ref["zeros"], (b, zeros, ref["zeros"])
    if np.isnan(ref["H"]):
        assert np.isnan(H) and np.isnan(knn).all(), b
        return
    rho2 = ref["rho2"]
    err = np.abs(knn.astype(LD) ** 2 - rho2)
    tol = 4 * (P + 2) * LD(2.0) ** -53 * rho2
    pos = rho2 > 0
    assert np.all(knn[~pos] == 0.0), b
    if pos.any():
        WORST["knn"] = max(WORST["knn"], float((err[pos] / tol[pos]).max()))
    assert np.all(err <= tol), (b, float((err[pos] / tol[pos]).max()))
    if ref["zeros"]:
        assert H == -np.inf, (b, H)
    else:
        bound = _h_bound(ref, P)
        e = abs(float(LD(H) - ref["H"]))
        WORST["H"] = max(WORST["H"], e / bound)
        assert e <= bound, (b, H, float(ref["H"]), e, bound)
    WORST["n"] += 1


# (P, K, k, B, method): every P, K <= 600, k and B of the docstring, both methods (method 1 with the rectangular kernel)
TARGET_CASES = [
    (2, 4, 4, 1, 0),                  # K = k: NaN
    (2, 5, 4, 3, 1),                  # K = k + 1
    (9, 9, 8, 3, 0),
    (3, 63, 1, 17, 0),
    (3, 64, 8, 3, 1),
    (16, 65, 4, 17, 1),
    (17, 255, 4, 3, 0),
    (16, 256, 1, 3, 0),
    (17, 257, 8, 1, 1),
    (5, 257, 4, 3, 1),
    (2, 600, 4, 17, 0),
]


@pytest.mark.parametrize("P,K,k,B,method", TARGET_CASES)
def test_targets_against_reference(ctx, P, K, k, B, method):
    F = _fit(ctx, P)
    T = F["T"][:B]
    vals, _, equal = _reference_rows(ctx, F, T, K, method, 1)
    assert equal.all()
    sd = F["Y"].std(axis=0, ddof=1)
    for entry, scale in (("targets_dev", None), ("targets_host", sd)):
        out = _ok(ctx, entry, K, k, F=F, targets=T, method=method, scale=scale)
        for b in range(B):
            _check_target(vals[b], out, b, k, scale)
    print("P=%d K=%d k=%d B=%d method %d: worst knn^2 %.3f, H %.4f of the bounds so far" % (P, K, k, B, method, WORST["knn"], WORST["H"]))


@pytest.mark.parametrize("K,P,k", [(8, 1, 8), (9, 1, 8), (2, 2, 1), (63, 3, 4), (64, 16, 4), (65, 17, 1), (255, 2, 8), (256, 17, 4),
                                   (257, 16, 8), (1000, 16, 4), (1000, 3, 1), (1000, 17, 4)])
def test_weighted_against_reference(ctx, K, P, k):
    """the generic entries, dense and through a strided view, with and without scale"""
    rng = np.random.default_rng(K + P)
    V = np.asfortranarray(rng.normal(size=(K, P)) * (1.0 + np.arange(P)))
    scale = 0.5 + np.arange(P)
    for entry, sc, pad in (("weighted_dev", None, 0), ("weighted_host", scale, 0), ("weighted_dev", scale, 7)):
        out = _ok(ctx, entry, K, k, V=V, scale=sc, pad=pad)
        _check_target(V, out, (), k, sc)


def test_invariance(ctx):
    """bit for bit: a repeat run, a target alone, the device against the host entry, a strided view, every member alone"""
    K = 65
    for P, method, k in ((3, 0, 4), (16, 1, 1), (17, 1, 8)):
        F = _fit(ctx, P)
        sd = F["Y"].std(axis=0, ddof=1)
        kw = dict(F=F, method=method, scale=sd)
        full = _ok(ctx, "targets_dev", K, k, targets=F["T"], **kw)
        again = _ok(ctx, "targets_dev", K, k, targets=F["T"], **kw)
        host = _ok(ctx, "targets_host", K, k, targets=F["T"], **kw)
        view = _ok(ctx, "targets_dev", K, k, targets=F["T"], pad=5, **kw)
        for m in MEMBERS:
            assert np.isfinite(full[m]).all(), (P, m)
            for other in (again, host, view):
                assert np.array_equal(other[m], full[m]), (P, m)
        for b in (0, 8, 16):
            for entry in ("targets_dev", "targets_host"):
                one = _ok(ctx, entry, K, k, targets=F["T"][b:b + 1], **kw)
                for m in MEMBERS:
                    assert np.array_equal(one[m][0], full[m][b]), (P, b, entry, m)
        rev = _ok(ctx, "targets_dev", K, k, targets=F["T"][::-1], **kw)
        for m in MEMBERS:
            assert np.array_equal(rev[m][::-1], full[m]), (P, m)
    # the generic entries: both paths, and every member alone on every entry
    V = np.random.default_rng(8).normal(size=(1000, 5))
    d, h = _ok(ctx, "weighted_dev", 1000, V=V), _ok(ctx, "weighted_host", 1000, V=V)
    for m in MEMBERS:
        assert np.array_equal(d[m], h[m]), m


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_member_alone(ctx, entry):
    rc, full = _small(ctx, entry)
    ctx.check(rc)
    for m in MEMBERS:
        assert np.isfinite(full[m]).all(), m
        rc, one = _small(ctx, entry, members=(m,))
        ctx.check(rc)
        assert np.array_equal(one[m], full[m]), m


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_first_call_on_a_fresh_context(ctx, entry):
    """each entry's reservation is sufficient on its own: no earlier call has grown the workspace"""
    from abcsmc_amd import _lib
    rc, warm = _small(ctx, entry)
    ctx.check(rc)
    fresh = _lib.Context(0)
    try:
        rc, first = _small(ctx, entry, fresh=fresh)
        fresh.check(rc)
    finally:
        fresh.close()
    for m in MEMBERS:
        assert np.array_equal(first[m], warm[m]), m


def test_permutation_scale_and_units(ctx):
    rng = np.random.default_rng(11)
    for K, P, k in ((300, 3, 4), (300, 17, 2)):
        V = rng.normal(size=(K, P)) * (1.0 + np.arange(P))
        base = _ok(ctx, "weighted_dev", K, k, V=V)
        # knn of the permuted rows is the permuted knn, bit for bit; zeros too; H only within its bound
        perm = rng.permutation(K)
        out = _ok(ctx, "weighted_dev", K, k, V=V[perm])
        assert np.array_equal(out["knn"], base["knn"][perm]) and out["zeros"] == base["zeros"]
        ref = R.entropy(V, k)
        assert abs(float(out["H"]) - float(base["H"])) <= _h_bound(ref, P)
        # scale against values divided beforehand: the same bits in every member
        scale = 0.3 + rng.uniform(size=P)
        a = _ok(ctx, "weighted_dev", K, k, V=V, scale=scale)
        b = _ok(ctx, "weighted_dev", K, k, V=V / scale)
        for m in MEMBERS:
            assert np.array_equal(a[m], b[m]), (P, m)
        # H(s V) - H(V) = P log s
        for s in (3.0, 0.001):
            hs = _ok(ctx, "weighted_host", K, k, V=s * V)["H"]
            assert abs(float(LD(hs) - LD(base["H"]) - P * np.log(LD(s)))) <= max(_h_bound(ref, P), _h_bound(R.entropy(s * V, k), P)), (P, s)


def test_duplicates(ctx):
    V = np.random.default_rng(12).normal(size=(70, 3))
    V[9] = V[55]
    for entry in ("weighted_dev", "weighted_host"):
        one = _ok(ctx, entry, 70, 1, V=V)
        assert one["zeros"] == 2 and one["H"] == -np.inf and one["knn"][9] == 0 and one["knn"][55] == 0
        assert (np.delete(one["knn"], (9, 55)) > 0).all()
        two = _ok(ctx, entry, 70, 2, V=V)
        assert two["zeros"] == 0 and np.isfinite(two["H"])
        _check_target(V, one, (), 1)
        _check_target(V, two, (), 2)


def test_nan_in_one_target_leaves_the_others(ctx):
    """a NaN in one parameter of one row: the targets that retain the row give NaN, every other target keeps its bits"""
    import torch
    from abcsmc_amd import device
    P, K = 4, 64
    F = _fit(ctx, P)
    T = F["T"]
    idx, _, _ = device.rank_targets(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, Y=F["Yd"], ctx=ctx)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy()
    row = idx[4, 3]
    hit = (idx == row).any(axis=1)
    assert hit[4] and not hit.all()
    for bad in (np.nan, np.inf):
        Y2 = F["Y"].copy()
        Y2[row, 2] = bad
        Y2d = device.colmajor(np.asfortranarray(Y2), DEV)
        base = _ok(ctx, "targets_dev", K, F=F, targets=T)
        out = _ok(ctx, "targets_dev", K, F=F, targets=T, Yd=Y2d)
        assert np.isnan(out["H"][hit]).all() and np.isnan(out["knn"][hit]).all() and (out["zeros"][hit] == 0).all()
        for m in MEMBERS:
            assert np.array_equal(out[m][~hit], base[m][~hit]), m
    V = np.random.default_rng(13).normal(size=(100, 17))
    V[3, 16] = np.nan
    out = _ok(ctx, "weighted_dev", 100, V=V)
    assert np.isnan(out["H"]) and np.isnan(out["knn"]).all() and out["zeros"] == 0


def test_method_1_sees_theta(ctx):
    """under transforms, the variance correction and the ridge adjustment the entropy is of the values theta holds: the generic
    entry on the returned theta gives the same bits"""
    import torch
    from abcsmc_amd import device
    P, K, B = 3, 100, 3
    F = _fit(ctx, P)
    Td = device.colmajor(F["T"][:B], DEV)
    lo, hi = F["Y"].min(axis=0) - 1.0, F["Y"].max(axis=0) + 1.0
    sd = F["Y"].std(axis=0, ddof=1)

    def both():
        r = device.rank_targets_entropy(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], k=4, scale=sd, method=1, adjust=("theta",), ctx=ctx)
        torch.cuda.synchronize()
        for b in range(B):
            g = device.weighted_entropy(r["theta"][b].T.contiguous(), k=4, scale=sd, ctx=ctx)
            torch.cuda.synchronize()
            for m in MEMBERS:
                assert np.array_equal(g[m].cpu().numpy(), r[m][b].cpu().numpy()), (b, m)
        return r["H"].cpu().numpy()

    plain = both()
    with ctx.param_transf(["logit", "none", "logit"], lo, hi):
        tf = both()
    with ctx.adjust_hcorr(True):
        hc = both()
    with ctx.adjust_ridge([0.1, 10.0]):
        rg = both()
    with ctx.param_transf(["logit", "none", "logit"], lo, hi), ctx.adjust_hcorr(True), ctx.adjust_ridge([0.1, 10.0]):
        every = both()
    assert np.isfinite(np.concatenate([plain, tf, hc, rg, every])).all()


def _small(ctx, entry, members=MEMBERS, fresh=None, **kw):
    """the call of the member / fresh-context / refusal tests: P = 3, 4 targets, K = 50, k = 4, method 1 (rectangular)"""
    F = _fit(ctx, 3)
    V = np.random.default_rng(5).normal(size=(50, 3))
    a = dict(F=F, targets=F["T"][:4], method=1) if entry.startswith("targets") else dict(V=V)
    a.update(members=members, scale=[1.0, 2.0, 0.5])
    a.update(kw)
    return _call(fresh if fresh is not None else ctx, entry, 50, **a)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals(ctx, entry):
    import torch
    from abcsmc_amd import _lib, device
    name = ENTRIES[entry]
    tg = entry.startswith("targets")
    last = lambda: _lib.lib().abc_last_error(ctx.handle).decode()
    F = _fit(ctx, 3)
    Td = device.colmajor(F["T"][:4], DEV)

    def plain():
        idx, dist, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, 50, Y=F["Yd"], ctx=ctx)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), dist.cpu().numpy()

    before = plain()
    rc, _ = _small(ctx, entry, null=True)
    assert rc == INVALID and last() == "%s: null argument (en is required)" % name
    for kw, text in ((dict(k=0), "k = 0 neighbours"), (dict(k=9), "k = 9 neighbours"), (dict(k=-1), "k = -1 neighbours"),
                     (dict(members=()), "every output member of en is NULL"), (dict(scale=[1.0, 0.0, 1.0]), "scale[1] = 0"),
                     (dict(scale=[-2.0, 1.0, 1.0]), "scale[0] = -2"), (dict(scale=[1.0, 1.0, np.nan]), "scale[2] = nan"),
                     (dict(scale=[1.0, np.inf, 1.0]), "scale[1] = inf")):
        rc, _ = _small(ctx, entry, **kw)
        assert rc == INVALID, kw
        assert last().startswith(name + ": ") and text in last(), (kw, last())
    if tg:
        rc, _ = _small(ctx, entry, kernel=0)                                 # method 1 with the Epanechnikov kernel
        assert rc == UNSUPPORTED and last().startswith(name + ": ") and "Epanechnikov" in last() and "rectangular" in last(), last()
        rc, out = _small(ctx, entry, method=0, kernel=0)                     # (method 0 does not weigh: any kernel)
        ctx.check(rc)
        with ctx.row_weights(np.linspace(0.5, 1.5, N)):
            for method in (0, 1):
                rc, _ = _small(ctx, entry, method=method)
                assert rc == UNSUPPORTED and last().startswith(name + ": ") and "row importance weights" in last(), last()
    else:
        rc, _ = _small(ctx, entry, w=np.ones(50))
        assert rc == UNSUPPORTED and last().startswith(name + ": ") and "weights w" in last(), last()
    after = plain()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    rc, out = _small(ctx, entry)
    ctx.check(rc)
    assert np.isfinite(out["H"]).all()


def test_retained_rows_are_more_concentrated_than_the_table(ctx):
    """over the 17 targets, the mean entropy of the K = 100 retained rows is below that of 100 rows taken evenly from the table"""
    F = _fit(ctx, 3)
    sd = F["Y"].std(axis=0, ddof=1)
    H = _ok(ctx, "targets_dev", 100, F=F, targets=F["T"], scale=sd)["H"]
    table = _ok(ctx, "weighted_dev", 100, V=F["Y"][::N // 100], scale=sd)["H"]
    print("mean entropy of the retained rows %.4f, of 100 rows of the table %.4f" % (H.mean(), float(table)))
    assert np.isfinite(H).all() and H.mean() < float(table)


def test_python_wrappers(ctx):
    """abcutil (host) and device (torch) give the entries' bits and shapes; the cross-validation and the component choice run"""
    import torch
    from abcsmc_amd import abcutil, device
    P, K, B = 5, 63, 3
    F = _fit(ctx, P)
    T = F["T"][:B]
    sd = F["Y"].std(axis=0, ddof=1)
    raw = _ok(ctx, "targets_dev", K, 3, F=F, targets=T, method=1, scale=sd)
    h = abcutil.particle_ranking_PLS_targets_entropy(F["X"], F["Y"], T, 0.5, K, k=3, scale="sd", method="loclinear", ctx=ctx)
    d = device.rank_targets_entropy(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"], k=3, scale=sd, method=1, ctx=ctx)
    torch.cuda.synchronize()
    assert h["H"].shape == (B,) and h["knn"].shape == (B, K) and h["zeros"].shape == (B,) and h["idx"].shape == (B, K)
    for m in MEMBERS:
        assert np.array_equal(h[m], raw[m].astype(h[m].dtype)), m
        assert np.array_equal(d[m].cpu().numpy(), raw[m]), m
    from abcsmc_amd import _lib
    for kw, text in ((dict(row_weights=np.ones(N)), "row importance weights"), (dict(method="loclinear", kernel="epanechnikov"), "Epanechnikov")):
        with pytest.raises(_lib.AbcError, match=text):                       # the wrappers hand on what the library refuses
            abcutil.particle_ranking_PLS_targets_entropy(F["X"], F["Y"], T, 0.5, K, ctx=ctx, **kw)
    V = np.random.default_rng(21).normal(size=(200, 4))
    g = abcutil.knn_entropy(V, k=2, scale=[1.0, 2.0, 3.0, 4.0], ctx=ctx)
    gd = device.weighted_entropy(device.colmajor(V, DEV), k=2, scale=[1.0, 2.0, 3.0, 4.0], ctx=ctx)
    torch.cuda.synchronize()
    rawg = _ok(ctx, "weighted_host", 200, 2, V=V, scale=[1.0, 2.0, 3.0, 4.0])
    assert g["knn"].shape == (200,) and np.ndim(g["H"]) == 0
    for m in MEMBERS:
        assert np.array_equal(g[m], rawg[m].astype(g[m].dtype)) and np.array_equal(gd[m].cpu().numpy(), rawg[m]), m
    # the cross-validation: the default call returns what it returned, entropy=True adds two members
    cv0 = abcutil.cross_validate_pls(F["X"], F["Y"], 10, 60, seed=3, ctx=ctx)
    cv = abcutil.cross_validate_pls(F["X"], F["Y"], 10, 60, seed=3, ctx=ctx, entropy=True)
    assert set(cv) == set(cv0) | {"entropy", "mean_entropy"} and "entropy" not in cv0
    for key in cv0:
        assert np.array_equal(cv[key], cv0[key]), key
    assert cv["entropy"].shape == (10,) and np.isfinite(cv["entropy"]).all() and cv["mean_entropy"] == float(cv["entropy"].mean())
    en = abcutil.particle_ranking_PLS_targets_entropy(F["X"], F["Y"], F["X"][cv["rows"]], 0.5, 60, scale="sd", exclude=cv["rows"], ctx=ctx)
    assert np.array_equal(en["H"], cv["entropy"])
    me = abcutil.min_entropy_components(F["X"], F["Y"], 10, 60, 3, [1, 2, 5], ctx=ctx)
    assert list(me["max_comp"]) == [1, 2, 5] and me["mean_entropy"].shape == (3,) and me["pred_error"].shape == (3, P)
    assert (me["ncomp"] <= me["max_comp"]).all() and me["best"] == me["max_comp"][int(np.argmin(me["mean_entropy"]))]
    cv3 = abcutil.cross_validate_pls(F["X"], F["Y"], 10, 60, seed=3, max_comp=2, ctx=ctx, entropy=True)
    assert me["mean_entropy"][1] == cv3["mean_entropy"] and me["ncomp"][1] == cv3["ncomp"]
    print("worst over %d targets: knn^2 %.3f of 4 (P + 2) 2^-53 rho2, H %.5f of its bound" % (WORST["n"], WORST["knn"], WORST["H"]))
