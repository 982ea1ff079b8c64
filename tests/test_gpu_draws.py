"""Posterior draws of the batched ranking (abc_rank_targets_draws_dev, abc_particle_ranking_pls_targets_draws, abc_weighted_draws*)
against the NumPy form of the header's definition (tests/_draws_ref.py), built on the device's own rows, adjusted values and weights.

Every case checks src against the reference wherever the reference does not call the draw ambiguous (tau within 4 K 2^-53 W of a
knot; at most 1 draw in 1000 may be, and with equal weights none), the plain draws bit for bit against the rows at the device's own
src, ess within K 2^-52 of the long-double value, and the smoothed draws within h_j zbound + 2 ulp(x) of the model at the device's
own src with bw_out bit for bit the density entry's.  Then the invariances the header states, the first call on a fresh context,
every member alone, the argument errors and the Python wrappers.

Sizes: 600 rows of 6 metrics; P = 3, 4, 5, 9 (below, at and above one Philox block of four parameters; three blocks); S = 1, 255,
256, 257, 4096 (DR_DB = 256 draws per work-group); K = 1, 2, 63, 64, 65, 257, 1000 and 1023, 1024, 1025 (DR_CH = 1024 entries per
chunk of the scan; the generic entry, which is not bound by the 600 rows); B = 1, 3, 17.

The worst |x_dev - x_ref| / (h zbound) and the ambiguous draws over the cases of this file are printed by test_python_wrappers
(run with -s).  They have not been recorded yet: no MI355X could be had when this file was written."""
import ctypes as C

import numpy as np
import pytest

import _draws_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, M = 600, 6
SEED = 0x0123456789ABCDEF
INVALID = -1
MEMBERS = ("draws", "src", "bw_out", "ess")
ENTRIES = {"targets_host": "abc_particle_ranking_pls_targets_draws", "targets_dev": "abc_rank_targets_draws_dev",
           "weighted_host": "abc_weighted_draws", "weighted_dev": "abc_weighted_draws_dev"}
LD = np.longdouble
WORST = {"z": 0.0, "amb": 0, "n": 0}        # largest |x_dev - x_ref| / (h zbound); ambiguous draws of all the draws compared


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


_FITS = {}


def _fit(ctx, P):
    """the set of P parameters, in host and device memory, its model for the device entries and 17 targets"""
    if P in _FITS:
        return _FITS[P]
    import torch
    from abcsmc_amd import _lib, device, synthetic
    wl = synthetic.Workload(M, P, 40 + P)
    X, Y = (np.asfortranarray(a) for a in wl.rows(0, N))
    A = min(M, P)
    L = _lib.lib()
    Xd, Yd = device.colmajor(X, DEV), device.colmajor(Y, DEV)
    stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=DEV)
    model = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=DEV)
    obs = torch.zeros(M, dtype=torch.float64, device=DEV)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
    ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, int(np.floor(0.5 * N + 0.5)),
                                         stats.data_ptr()))
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), obs.data_ptr(), M, P, A, 0, model.data_ptr()))
    torch.cuda.synchronize()
    rows = (np.arange(17) * 31 + 5) % N
    _FITS[P] = dict(X=X, Y=Y, Xd=Xd, Yd=Yd, model=model, A=A, P=P, T=np.asfortranarray(X[rows]))
    return _FITS[P]


def _shapes(lead, S, P):
    return dict(draws=lead + (S, P), src=lead + (S,), bw_out=lead + (P,), ess=lead)


def _call(ctx, entry, S, K, F=None, targets=None, Yd=None, V=None, w=None, smooth=0, seed=SEED, stream=None, members=MEMBERS,
          method=0, kernel=0, bw=None, bw_scale=1.0, null=False):
    """One call of an entry straight through ctypes with exactly `members` of the descriptor's outputs non-NULL (null: a NULL
    descriptor).  targets entries: F (the fit) and targets (B, M); weighted entries: V (K, P) and w (K,) or None.  bw: host array
    shaped as bw_out.  Every output starts as NaN / all ones.  -> (status, {member: numpy array})"""
    import torch
    from abcsmc_amd import _lib, device
    on_dev, tg = entry.endswith("_dev"), entry.startswith("targets")
    if tg:
        B, P = targets.shape[0], F["P"]
        lead = (B,)
    else:
        V = np.asfortranarray(V)
        P, lead = V.shape[1], ()
    keep, out = [], {}
    for k in members:
        shape = _shapes(lead, S, P)[k]
        if k == "src":
            out[k] = torch.full(shape, -1, dtype=torch.int64, device=DEV) if on_dev else np.full(shape, 2 ** 64 - 1, dtype=np.uint64)
        else:
            out[k] = torch.full(shape, np.nan, dtype=torch.float64, device=DEV) if on_dev else np.full(shape, np.nan)
    p = (lambda t: t.data_ptr()) if on_dev else (lambda v: v.ctypes.data)
    o = lambda k: p(out[k]) if k in out else None
    bwp = None
    if bw is not None:
        bwa = np.ascontiguousarray(bw, dtype=np.float64)
        bwa = torch.tensor(bwa, device=DEV) if on_dev else bwa
        keep.append(bwa)
        bwp = p(bwa)
    ids = None if stream is None else np.ascontiguousarray(stream, dtype=np.uint64).reshape(-1)
    desc = _lib.Draws(S, smooth, bw_scale, bwp, seed, None if ids is None else ids.ctypes.data, o("draws"), o("src"), o("bw_out"),
                      o("ess"))
    ref = None if null else C.byref(desc)
    fn = getattr(_lib.lib(), ENTRIES[entry])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if entry == "targets_host":
        T = np.asfortranarray(targets)
        rc = fn(ctx.handle, F["X"].ctypes.data, F["Y"].ctypes.data, N, M, P, T.ctypes.data, B, 0.5, 0, 0, None, K, method, kernel,
                None, None, None, ref, None)
    elif entry == "targets_dev":
        Td = device.colmajor(np.asfortranarray(targets), DEV)
        Yd = F["Yd"] if Yd is None else Yd
        rc = fn(ctx.handle, F["Xd"].data_ptr(), N, Yd.data_ptr(), N, N, M, P, F["model"].data_ptr(), F["A"], Td.data_ptr(), B, B,
                None, K, method, kernel, None, None, None, ref)
    elif entry == "weighted_host":
        wa = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        rc = fn(ctx.handle, V.ctypes.data, K, P, None if wa is None else wa.ctypes.data, ref)
    else:
        Vd = device.colmajor(V, DEV)
        wd = None if w is None else torch.tensor(np.ascontiguousarray(w, dtype=np.float64), device=DEV)
        rc = fn(ctx.handle, Vd.data_ptr(), K, K, P, None if wd is None else wd.data_ptr(), ref)
    if on_dev:
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    if "src" in out:
        out["src"] = out["src"].astype(np.int64)
    return rc, out


def _ok(ctx, *a, **kw):
    rc, out = _call(ctx, *a, **kw)
    ctx.check(rc)
    return out


def _check_target(vals, wts, out, b, K, S, seed, stream, h, equal):
    """target b of the outputs (out[name][b]; b = () for the generic entries) against the reference.  vals: (K, P) the target's
    rows in ranking order, wts: (K,) or None, h: (P,) the bandwidths expected in bw_out (None: plain draws), equal: the weights
    are equal, so src is exact"""
    src, x, ess = out["src"][b], out["draws"][b], out["ess"][b]
    assert src.min() >= 0 and src.max() <= K - 1
    rsrc, amb = R.select(None if equal else wts, K, seed, stream, S)
    WORST["amb"] += int(amb.sum())
    WORST["n"] += S
    assert np.array_equal(src[~amb], rsrc[~amb]), (b, int((src != rsrc).sum()))
    if wts is not None:
        assert np.all(wts[src] > 0), b
    e_ref = R.ess(wts, K)
    assert abs(LD(ess) - e_ref) <= K * 2.0 ** -52 * e_ref, (b, ess, e_ref)
    v = vals[src]
    if h is None:
        assert np.isnan(out["bw_out"][b]).all()
        assert np.array_equal(x.view(np.uint64), v.view(np.uint64)), b
        return int(amb.sum())
    assert np.array_equal(out["bw_out"][b].view(np.uint64), np.asarray(h).view(np.uint64)), (b, out["bw_out"][b], h)
    z, zb = R.noise(seed, stream, S, vals.shape[1])
    good = np.isfinite(h)
    assert np.isnan(x[:, ~good]).all()
    x_ref = (h.astype(LD) * z + v).astype(np.float64)
    err = np.abs(x - x_ref)[:, good]
    zb_abs = (np.abs(h) * zb)[:, good]
    tol = zb_abs + 2.0 * np.spacing(np.abs(x_ref[:, good]))
    if err.size:
        WORST["z"] = max(WORST["z"], float((err[zb_abs > 0] / zb_abs[zb_abs > 0]).max()))
    assert np.all(err <= tol), (b, float((err / tol).max()))
    return int(amb.sum())


def _reference_rows(ctx, F, targets, K, method, kernel):
    """(vals (B, K, P), wts (B, K) or None, equal (B,)) of the targets entries, from the plain ranking or the adjustment's outputs"""
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(np.asfortranarray(targets), DEV)
    B = targets.shape[0]
    if method == 0:
        idx, _, _ = device.rank_targets(F["Xd"], F["model"], F["A"], Td, K, Y=F["Yd"], ctx=ctx)
        torch.cuda.synchronize()
        return F["Y"][idx.cpu().numpy()], None, np.ones(B, dtype=bool)
    r = device.rank_targets_adjust(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], kernel=kernel, ctx=ctx)
    torch.cuda.synchronize()
    th, wt, st = r["theta"].cpu().numpy(), r["weight"].cpu().numpy(), r["status"].cpu().numpy()
    return th, wt, (kernel == 1) | ((st & 2) != 0)


def _density_bw(ctx, F, targets, K, method, kernel, bw_scale):
    import torch
    from abcsmc_amd import device
    Td = device.colmajor(np.asfortranarray(targets), DEV)
    r = device.rank_targets_density(F["Xd"], F["model"], F["A"], Td, K, F["Yd"], G=16, bw_scale=bw_scale, method=method, kernel=kernel,
                                    dens=False, mode=False, ctx=ctx)
    torch.cuda.synchronize()
    return r["bw"].cpu().numpy()


# (P, K, S, B, method, kernel, smooth): every P, K <= 600, S and B of the docstring, both methods, kernels and kinds of draws
TARGET_CASES = [
    (3, 1, 1, 1, 0, 0, 0),
    (3, 1, 255, 3, 1, 0, 1),          # K = 1: the rectangular fallback
    (4, 2, 256, 17, 1, 0, 0),
    (5, 2, 257, 3, 0, 1, 1),
    (9, 63, 4096, 3, 1, 0, 1),
    (3, 64, 4096, 17, 1, 0, 0),
    (4, 65, 257, 17, 1, 1, 1),
    (5, 257, 4096, 17, 1, 0, 1),
    (9, 257, 255, 1, 0, 0, 0),
    (4, 600, 256, 3, 1, 0, 0),
    (3, 257, 1, 17, 0, 0, 1),
]


@pytest.mark.parametrize("P,K,S,B,method,kernel,smooth", TARGET_CASES)
def test_targets_against_reference(ctx, P, K, S, B, method, kernel, smooth):
    F = _fit(ctx, P)
    T = F["T"][:B]
    out = _ok(ctx, "targets_dev", S, K, F=F, targets=T, method=method, kernel=kernel, smooth=smooth, bw_scale=0.7)
    vals, wts, equal = _reference_rows(ctx, F, T, K, method, kernel)
    h = _density_bw(ctx, F, T, K, method, kernel, 0.7) if smooth else None
    amb = 0
    for b in range(B):
        amb += _check_target(vals[b], None if wts is None else wts[b], out, b, K, S, SEED, b, None if h is None else h[b], equal[b])
        if wts is not None and not equal[b]:
            assert wts[b, K - 1] == 0.0 and K - 1 not in out["src"][b]        # the Epanechnikov weight at the bandwidth
    print("P=%d K=%d S=%d B=%d method %d kernel %d smooth %d: %d of %d draws ambiguous" % (P, K, S, B, method, kernel, smooth, amb, B * S))
    assert amb * 1000 <= B * S


@pytest.mark.parametrize("K,P,S", [(1, 3, 1), (2, 4, 256), (63, 9, 4096), (64, 3, 255), (65, 5, 257), (257, 4, 256), (1000, 5, 4096),
                                   (1023, 9, 257), (1024, 3, 255), (1025, 4, 4096), (2049, 5, 257)])
def test_weighted_against_reference(ctx, K, P, S):
    """the generic entry with weights (zeros at both ends and in the middle), without, and smoothed with given and ruled bandwidths"""
    from abcsmc_amd import abcutil
    rng = np.random.default_rng(K)
    V = np.asfortranarray(rng.normal(size=(K, P)) * (1.0 + np.arange(P)))
    d = rng.uniform(0.0, 1.0, size=K)
    w = 1.0 - d * d                                                        # Epanechnikov weights of random distances
    if K >= 63:
        w[0] = w[K // 2] = w[K - 1] = 0.0
    amb = 0
    for entry in ("weighted_dev", "weighted_host"):
        for wts in (w, None):
            out = _ok(ctx, entry, S, K, V=V, w=wts, stream=[7])
            amb += _check_target(V, wts, out, (), K, S, SEED, 7, None, wts is None)
            if wts is not None and K >= 63:
                assert not np.isin(out["src"], (0, K // 2, K - 1)).any()
    # smoothed: the rule's bandwidths are the density entry's bits; given bandwidths are used as they are
    h = abcutil.weighted_density(V, w, G=16, bw_scale=1.3, ctx=ctx)["bw"]
    out = _ok(ctx, "weighted_dev", S, K, V=V, w=w, smooth=1, bw_scale=1.3, stream=[1 << 33])
    amb += _check_target(V, w, out, (), K, S, SEED, 1 << 33, h, False)
    given = np.linspace(0.1, 2.0, P)
    out = _ok(ctx, "weighted_host", S, K, V=V, w=None, smooth=1, bw=given, seed=5)
    amb += _check_target(V, None, out, (), K, S, 5, 0, given, True)
    print("K=%d P=%d S=%d: %d of %d draws ambiguous" % (K, P, S, amb, 6 * S))
    assert amb * 1000 <= 6 * S


def test_invariance(ctx):
    """bit for bit: a repeat run, a target alone under its stream id, device against host entry, S = 100 as the prefix of S = 257"""
    K, S = 65, 257
    for P, method, smooth in ((5, 1, 1), (3, 0, 0), (4, 0, 1), (9, 1, 0)):
        F = _fit(ctx, P)
        kw = dict(F=F, method=method, smooth=smooth, bw_scale=0.9)
        full = _ok(ctx, "targets_dev", S, K, targets=F["T"], **kw)
        again = _ok(ctx, "targets_dev", S, K, targets=F["T"], **kw)
        host = _ok(ctx, "targets_host", S, K, targets=F["T"], **kw)
        short = _ok(ctx, "targets_dev", 100, K, targets=F["T"], **kw)
        for k in MEMBERS:
            assert np.array_equal(again[k], full[k], equal_nan=True), (P, k)
            assert np.array_equal(host[k], full[k], equal_nan=True), (P, k)
        assert np.array_equal(short["draws"], full["draws"][:, :100]) and np.array_equal(short["src"], full["src"][:, :100])
        assert np.array_equal(short["ess"], full["ess"]) and np.array_equal(short["bw_out"], full["bw_out"], equal_nan=True)
        for b in (0, 8, 16):
            for entry in ("targets_dev", "targets_host"):
                one = _ok(ctx, entry, S, K, targets=F["T"][b:b + 1], stream=[b], **kw)
                for k in MEMBERS:
                    assert np.array_equal(one[k][0], full[k][b], equal_nan=True), (P, b, entry, k)
        # the stream id, not the position in the batch, addresses the draws: the batch reversed under the same ids
        rev = _ok(ctx, "targets_dev", S, K, targets=F["T"][::-1], stream=np.arange(17)[::-1], **kw)
        for k in MEMBERS:
            assert np.array_equal(rev[k][::-1], full[k], equal_nan=True), (P, k)
        other = _ok(ctx, "targets_dev", S, K, targets=F["T"][:1], stream=[3], **kw)
        assert not np.array_equal(other["src"][0], full["src"][0])
    # the generic entries
    rng = np.random.default_rng(8)
    V, w = rng.normal(size=(1025, 5)), rng.uniform(0, 1, size=1025)
    for smooth in (0, 1):
        d = _ok(ctx, "weighted_dev", S, 1025, V=V, w=w, smooth=smooth)
        h = _ok(ctx, "weighted_host", S, 1025, V=V, w=w, smooth=smooth)
        short = _ok(ctx, "weighted_host", 100, 1025, V=V, w=w, smooth=smooth)
        for k in MEMBERS:
            assert np.array_equal(d[k], h[k], equal_nan=True), k
        assert np.array_equal(short["draws"], d["draws"][:100]) and np.array_equal(short["src"], d["src"][:100])


def test_nan_parameter_leaves_the_others(ctx):
    """a NaN in one parameter of one row: the smoothed draws of that parameter are NaN for the targets that retain the row, the
    plain draws carry the NaN only where the row is drawn, and every other segment keeps its bits"""
    import torch
    from abcsmc_amd import device
    P, K, S, j0 = 4, 64, 257, 2
    F = _fit(ctx, P)
    T = F["T"]
    idx, _, _ = device.rank_targets(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, Y=F["Yd"], ctx=ctx)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy()
    row = idx[4, 3]
    hit = (idx == row).any(axis=1)                                         # the targets that retain the row
    assert hit[4] and not hit.all()
    Y2 = F["Y"].copy()
    Y2[row, j0] = np.nan
    Y2d = device.colmajor(np.asfortranarray(Y2), DEV)
    for smooth in (0, 1):
        base = _ok(ctx, "targets_dev", S, K, F=F, targets=T, smooth=smooth)
        out = _ok(ctx, "targets_dev", S, K, F=F, targets=T, Yd=Y2d, smooth=smooth)
        assert np.array_equal(out["src"], base["src"]) and np.array_equal(out["ess"], base["ess"])
        same = np.ones((17, P), dtype=bool)
        same[hit, j0] = False
        for b in range(17):
            for j in range(P):
                if same[b, j]:
                    assert np.array_equal(out["draws"][b, :, j], base["draws"][b, :, j]), (smooth, b, j)
                    assert np.array_equal(out["bw_out"][b, j], base["bw_out"][b, j], equal_nan=True), (smooth, b, j)
                elif smooth:
                    assert np.isnan(out["bw_out"][b, j]) and np.isnan(out["draws"][b, :, j]).all(), (b, j)
                else:
                    from_row = idx[b][out["src"][b]] == row
                    assert np.array_equal(np.isnan(out["draws"][b, :, j]), from_row), (b, j)
                    assert np.array_equal(out["draws"][b, ~from_row, j], base["draws"][b, ~from_row, j]), (b, j)
    # the generic entry: a NaN in one column
    rng = np.random.default_rng(9)
    V, w = rng.normal(size=(300, 5)), rng.uniform(0, 1, size=300)
    V2 = V.copy()
    V2[17, 3] = np.nan
    base = _ok(ctx, "weighted_dev", S, 300, V=V, w=w, smooth=1)
    out = _ok(ctx, "weighted_dev", S, 300, V=V2, w=w, smooth=1)
    keep = [0, 1, 2, 4]
    assert np.array_equal(out["draws"][:, keep], base["draws"][:, keep]) and np.isnan(out["draws"][:, 3]).all()
    assert np.array_equal(out["bw_out"][keep], base["bw_out"][keep]) and np.isnan(out["bw_out"][3])
    assert np.array_equal(out["src"], base["src"])


def _small(ctx, entry, members=MEMBERS, fresh=None, **kw):
    """the call of the member / fresh-context / error tests: P = 3, 4 targets, K = 50, S = 300, method 1, smoothed"""
    F = _fit(ctx, 3)
    rng = np.random.default_rng(5)
    V, w = rng.normal(size=(50, 3)), rng.uniform(0.1, 1.0, size=50)
    a = dict(F=F, targets=F["T"][:4], method=1) if entry.startswith("targets") else dict(V=V, w=w)
    a.update(smooth=1, members=members)
    a.update(kw)
    S = a.pop("S", 300)
    return _call(fresh if fresh is not None else ctx, entry, S, 50, **a)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_member_alone(ctx, entry):
    rc, full = _small(ctx, entry)
    ctx.check(rc)
    for k in MEMBERS:
        assert np.isfinite(full[k]).all(), k
        rc, one = _small(ctx, entry, members=(k,))
        ctx.check(rc)
        assert np.array_equal(one[k], full[k]), k
    rc, plain = _small(ctx, entry, smooth=0)
    ctx.check(rc)
    for k in ("src", "ess"):                                               # the selection does not depend on the smoothing
        assert np.array_equal(plain[k], full[k]), k
        rc, one = _small(ctx, entry, members=(k,), smooth=0)
        ctx.check(rc)
        assert np.array_equal(one[k], plain[k]), k


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
    for k in MEMBERS:
        assert np.array_equal(first[k], warm[k]), k


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_argument_errors(ctx, entry):
    from abcsmc_amd import _lib
    name = ENTRIES[entry]
    last = lambda: _lib.lib().abc_last_error(ctx.handle).decode()
    rc, _ = _small(ctx, entry, null=True)
    assert rc == INVALID and last() == "%s: null argument (dr is required)" % name
    for kw, text in ((dict(S=0), "S = 0 draws"), (dict(S=(1 << 24) + 1), "S = 16777217 draws"), (dict(smooth=2), "smooth 2"),
                     (dict(smooth=-1), "smooth -1"), (dict(members=()), "every output member of dr is NULL"),
                     (dict(bw_scale=0.0), "bw_scale = 0"), (dict(bw_scale=-1.0), "bw_scale = -1"),
                     (dict(bw_scale=float("nan")), "bw_scale = nan"), (dict(bw_scale=float("inf")), "bw_scale = inf")):
        if "S" in kw and kw["S"] > 1:
            kw = dict(kw, members=("ess",))                                # (no output of 2^24 draws is allocated for the check)
        rc, _ = _small(ctx, entry, **kw)
        assert rc == INVALID, kw
        assert last().startswith(name + ": ") and text in last(), (kw, last())
    lead = (4,) if entry.startswith("targets") else ()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        bw = np.ones(lead + (3,))
        bw[..., 1] = bad
        rc, _ = _small(ctx, entry, bw=bw)
        assert rc == INVALID, bad
        assert last() == "%s: a given bandwidth is not finite and positive" % name
    # without smoothing neither bw_scale nor bw is looked at
    rc, out = _small(ctx, entry, smooth=0, bw_scale=-1.0)
    ctx.check(rc)
    assert np.isnan(out["bw_out"]).all()


def test_python_wrappers(ctx):
    """abcutil (host) and device (torch) give the entries' bits and shapes"""
    import torch
    from abcsmc_amd import abcutil, device
    P, K, S, B = 5, 63, 300, 3
    F = _fit(ctx, P)
    T = F["T"][:B]
    ids = [5, 1 << 40, 9]
    raw = _ok(ctx, "targets_dev", S, K, F=F, targets=T, method=1, smooth=1, stream=ids, seed=77)
    h = abcutil.particle_ranking_PLS_targets_draws(F["X"], F["Y"], T, 0.5, K, S, smooth=True, seed=77, method="loclinear", stream=ids,
                                                   ctx=ctx)
    d = device.rank_targets_draws(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"], S, smooth=True, seed=77,
                                  stream=ids, method=1, ctx=ctx)
    torch.cuda.synchronize()
    assert h["draws"].shape == (B, S, P) and h["src"].shape == (B, S) and h["ess"].shape == (B,) and h["bw"].shape == (B, P)
    for k, name in (("draws", "draws"), ("src", "src"), ("bw_out", "bw"), ("ess", "ess")):
        assert np.array_equal(np.asarray(h[name]).astype(raw[k].dtype), raw[k]), k
        assert np.array_equal(d[name].cpu().numpy(), raw[k]), k
    rng = np.random.default_rng(3)
    V, w = rng.normal(size=(200, P)), rng.uniform(0, 1, size=200)
    raw = _ok(ctx, "weighted_host", S, 200, V=V, w=w, seed=3)
    hw = abcutil.weighted_draws(V, w, S=S, seed=3, ctx=ctx)
    dw = device.weighted_draws(torch.tensor(V.T.copy(), device=DEV), torch.tensor(w), S=S, seed=3, ctx=ctx)
    torch.cuda.synchronize()
    for k, name in (("draws", "draws"), ("src", "src"), ("ess", "ess")):
        assert np.array_equal(np.asarray(hw[name]).astype(raw[k].dtype), raw[k]), k
        assert np.array_equal(dw[name].cpu().numpy(), raw[k]), k
    assert np.isnan(hw["bw"]).all() and np.array_equal(hw["draws"], V[hw["src"].astype(np.int64)])
    print("over this file so far: worst |x_dev - x_ref| / (h zbound) %.3g; %d of %d draws ambiguous" % (WORST["z"], WORST["amb"],
                                                                                                       WORST["n"]))
