"""The sufficient-statistics record (abc_stats_shift_dev + abc_stats_accumulate_dev) of every statistics kernel against an exact
reference of the same operation, called through the C ABI with the record buffer filled with NaN first, so that an entry a kernel
fails to write shows up.

Reference: the shift is the mean of the first min(n, 256) rows by math.fsum; V = Z - shift in fp64, formed with the DEVICE's shift
exactly as the kernels form it; sums and Gram of V per partition in long double (80-bit here), the Gram as fp64 products of
32-row chunks summed in long double: its own error is at most 32 u sum_r |v_ra v_rb| <= 3.6e-15 sqrt(G_aa G_bb).
Bounds (the header promises ~1e-15 for the fp64 kernels):
    counts exact; shift within 2 ulp of the largest |value| of the pilot rows; sums within 1e-13 sum |v|;
    Gram entries of the X'X block, the X'Y block and the Y'Y diagonal within 1e-13 sqrt(G_aa G_bb);
    Y'Y entries off the diagonal either within that bound or, inside the 16-column blocks the fp64 kernels skip, exactly 0;
    padding columns M+P .. C16 exactly 0; the Gram symmetric bit for bit; no NaN anywhere.
Every case states, through tests/_gram_dispatch.py, the kernel family and instantiation it reaches.  The byte-limb kernel (i8) is
held to its own error model in tests/test_gpu_parity.py::test_wide_gram_on_the_i8_matrix_pipe."""
import math

import numpy as np
import pytest

from _gram_dispatch import kernel_for, plan, work_groups

pytestmark = pytest.mark.gpu

TOL = 1e-13
CHUNK = 32


# ---------------------------------------------------------------------------------------------------------------------------------
# device buffers, the record, the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _dev_cols(A, ld, off):
    """A (n x k) as k columns of leading dimension ld, off doubles after the allocation's start; rows [n, ld) NaN.
    -> (tensor, address of the first column)"""
    import torch
    n, k = A.shape
    t = torch.full((off + ld * max(k, 1),), float("nan"), dtype=torch.float64, device="cuda:0")
    if n and k:
        t[off:off + ld * k].view(k, ld)[:, :n] = torch.from_numpy(np.ascontiguousarray(A.T)).to("cuda:0")
    return t, t.data_ptr() + 8 * off


def _record(gpu_ctx, X, Y, ntrain, ldx=None, ldy=None, xoff=0, yoff=0):
    """abc_stats_shift_dev + abc_stats_accumulate_dev into a NaN-filled record -> numpy record"""
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    n, M = X.shape
    P = Y.shape[1]
    ldx = n if ldx is None else ldx
    ldy = n if ldy is None else ldy
    tX, pX = _dev_cols(X, ldx, xoff)
    tY, pY = _dev_cols(Y, ldy, yoff)
    st = torch.full((L.abc_stats_len(M, P),), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.check(L.abc_stats_shift_dev(gpu_ctx.handle, pX, pY, n, ldx, ldy, M, P, st.data_ptr()))
    gpu_ctx.check(L.abc_stats_accumulate_dev(gpu_ctx.handle, pX, pY, n, ldx, ldy, M, P, 0, ntrain, st.data_ptr()))
    torch.cuda.synchronize()
    return st.cpu().numpy()


def _parts(rec, C16):
    """record -> (counts, shift, [sum_train, sum_test], [G_train, G_test]) (views)"""
    G0 = 2 + 3 * C16
    return (rec[0:2], rec[2:2 + C16], [rec[2 + C16:2 + 2 * C16], rec[2 + 2 * C16:2 + 3 * C16]],
            [rec[G0:G0 + C16 * C16].reshape(C16, C16).T, rec[G0 + C16 * C16:G0 + 2 * C16 * C16].reshape(C16, C16).T])


def _gram_ld(V):
    """V'V: fp64 products of CHUNK-row chunks, summed in long double"""
    n, k = V.shape
    G = np.zeros((k, k), dtype=np.longdouble)
    nb = -(-n // CHUNK)
    if not n:
        return G
    Vp = np.zeros((nb * CHUNK, k))
    Vp[:n] = V
    B = Vp.reshape(nb, CHUNK, k)
    for c0 in range(0, nb, 1024):
        b = B[c0:c0 + 1024]
        G += np.matmul(b.transpose(0, 2, 1), b).astype(np.longdouble).sum(axis=0)
    return G


def _reference(Z, shift, split):
    """per partition: (sums, sums of |v|, Gram) of V = Z - shift, long double"""
    assert np.finfo(np.longdouble).eps < 1e-18, "the reference needs an extended long double"
    V = Z - shift
    out = []
    for a, b in ((0, split), (split, Z.shape[0])):
        Vp = V[a:b]
        out.append((Vp.astype(np.longdouble).sum(axis=0), np.abs(Vp).astype(np.longdouble).sum(axis=0), _gram_ld(Vp)))
    return out


def _pilot_mean(Z):
    m = min(Z.shape[0], 256)
    if not m:
        return np.zeros(Z.shape[1]), np.zeros(Z.shape[1])
    return (np.array([math.fsum(Z[:m, c]) / m for c in range(Z.shape[1])]), np.abs(Z[:m]).max(axis=0))


def _check(rec, X, Y, split, fam, C, CY, check_shift=True):
    """every entry of the record against the exact reference; -> the reference (for reuse)"""
    n, M = X.shape
    P = Y.shape[1]
    K, C16 = M + P, 16 * C
    Z = np.hstack([X, Y])
    assert not np.isnan(rec).any(), "NaN left in the record at %s" % (np.nonzero(np.isnan(rec))[0][:10],)
    counts, shift, sums, G = _parts(rec, C16)
    assert counts[0] == split and counts[1] == n - split, counts
    if check_shift:
        mean, mag = _pilot_mean(Z)
        err = np.abs(shift[:K] - mean)
        assert np.all(err <= 2 * np.spacing(mag)), (np.argmax(err / (np.spacing(mag) + 1e-300)), err.max())
    assert np.all(shift[K:] == 0)
    refs = _reference(Z, shift[:K], split)
    skipped = np.zeros((K, K), dtype=bool)        # off-diagonal entries of the pure-Y 16-column blocks the fp64 kernels skip
    if not fam.startswith("grouped") and CY:
        y0 = 16 * (C - CY)
        skipped[y0:, y0:] = True
        np.fill_diagonal(skipped, False)
    for part in (0, 1):
        s_ref, a_ref, G_ref = refs[part]
        s, g = sums[part], G[part]
        serr = np.abs(s[:K].astype(np.longdouble) - s_ref)
        assert np.all(serr <= TOL * a_ref), (part, int(np.argmax(serr - TOL * a_ref)), float(serr.max()))
        assert np.all(s[K:] == 0), part
        d = np.diag(G_ref)
        scale = np.sqrt(np.outer(d, d))
        gerr = np.abs(g[:K, :K].astype(np.longdouble) - G_ref)
        bad = (gerr > TOL * scale) & ~skipped
        assert not bad.any(), "partition %d: %d entries off, first at %s: %r against %r" % (
            part, int(bad.sum()), np.argwhere(bad)[0], g[tuple(np.argwhere(bad)[0])], G_ref[tuple(np.argwhere(bad)[0])])
        assert np.all(g[:K, :K][skipped] == 0), part
        assert np.all(g[K:, :] == 0) and np.all(g[:, K:] == 0), "padding of partition %d not zero" % part
        assert np.array_equal(g, g.T), "partition %d: Gram not symmetric bit for bit" % part
    return refs


def _data(n, M, P, seed, kind="plain"):
    """columns of assorted centres and scales with some correlation; kinds plant the awkward ones"""
    rng = np.random.default_rng(seed)
    K = M + P
    f = rng.normal(size=(n, 1))
    Z = rng.normal(size=(n, K)) + 0.6 * f * rng.normal(size=K)
    Z = Z * np.exp(rng.uniform(-3, 3, size=K)) + rng.normal(size=K) * 10.0 ** rng.uniform(-1, 3, size=K)
    if kind == "constant":
        Z[:, 1] = 3.25
        Z[:, K - 1] = 0.1
    elif kind == "far":                       # a column 1e7 sigma from zero
        Z[:, 0] = 1e7 + rng.normal(size=n)
        Z[:, M] = -3e9 + 300.0 * rng.normal(size=n)
    elif kind == "pilot":                     # an unrepresentative pilot: the first 256 rows 1e3 sigma away from the rest
        Z[:256] += 1e3 * Z.std(axis=0)
    return np.asfortranarray(Z[:, :M]), np.asfortranarray(Z[:, M:])


def _case(gpu_ctx, M, P, n, split, expect, ldx=None, ldy=None, xoff=0, yoff=0, kind="plain", seed=1):
    X, Y = _data(n, M, P, seed, kind)
    fam, C, CY = kernel_for(M, P, n, split, ldx, ldy, 8 * xoff, 8 * yoff)
    assert (fam, C, CY) == expect, ((fam, C, CY), expect)
    rec = _record(gpu_ctx, X, Y, split, ldx, ldy, xoff, yoff)
    _check(rec, X, Y, split, fam, C, CY)
    return X, Y, rec


# ---------------------------------------------------------------------------------------------------------------------------------
# every instantiation of the fp64 families, and both branches of the grouped path at 7 and at more than 10 column blocks
# ---------------------------------------------------------------------------------------------------------------------------------
_O = 1        # one-double offset of a base pointer (8 bytes)
INSTANCES = [
    # M, P, n, split, expected, ldx, ldy, xoff, yoff
    (5, 3, 3001, 1500, ("vgpr", 1, 0), None, None, 0, 0),
    (20, 8, 2000, 1000, ("vgpr", 2, 0), None, None, 0, 0),
    (10, 16, 2000, 1281, ("vgpr", 2, 1), None, None, 0, 0),
    (40, 8, 2000, 1000, ("vgpr", 3, 0), None, None, 0, 0),
    (20, 20, 2001, 1001, ("vgpr", 3, 1), None, None, 0, 0),
    (7, 30, 2000, 1000, ("vgpr", 3, 2), None, None, 0, 0),
    (50, 10, 2001, 1000, ("vgpr", 4, 0), None, None, 0, 0),                   # odd n
    (40, 20, 2000, 1000, ("vgpr", 4, 1), 2001, 2002, 0, 0),                   # odd ldx
    (20, 40, 2000, 1000, ("vgpr", 4, 2), None, None, _O, 0),                  # X 8 bytes off
    (70, 9, 2001, 999, ("vgpr", 5, 0), None, None, 0, 0),
    (50, 30, 2000, 1000, ("vgpr", 5, 1), 2064, 2065, 0, 0),                   # odd ldy
    (40, 40, 2000, 1000, ("vgpr", 5, 2), None, None, 0, _O),                  # Y 8 bytes off
    (90, 6, 2000, 1000, ("vgpr", 6, 0), None, None, 0, 0),
    (70, 20, 2001, 1000, ("vgpr", 6, 1), None, None, 0, 0),
    (64, 32, 2001, 1000, ("vgpr", 6, 2), None, None, 0, 0),
    (50, 10, 2000, 1000, ("dma8", 4, 0), None, None, 0, 0),
    (40, 20, 2000, 1001, ("dma8", 4, 1), 2002, 2064, 0, 0),
    (20, 40, 2000, 1000, ("dma8", 4, 2), None, None, 0, 0),
    (70, 9, 2000, 1024, ("dma8", 5, 0), None, None, 0, 0),
    (50, 30, 2000, 1000, ("dma8", 5, 1), 2064, 2002, 0, 0),
    (40, 40, 2000, 999, ("dma8", 5, 2), None, None, 0, 0),
    (70, 20, 2000, 1000, ("dma8", 6, 1), None, None, 0, 0),
    (64, 32, 2000, 1000, ("dma8", 6, 2), None, None, 0, 0),
    (120, 8, 2000, 1000, ("wide", 8, 0), None, None, 0, 0),
    (100, 28, 2001, 1000, ("wide", 8, 1), None, None, 0, 0),
    (89, 36, 2000, 1000, ("wide", 8, 2), 2001, 2002, 0, 0),
    (131, 6, 2000, 1000, ("wide", 9, 0), None, None, 0, 0),
    (128, 16, 2000, 1000, ("wide", 9, 1), None, None, _O, 0),
    (105, 36, 2000, 1000, ("wide", 9, 2), None, None, 0, 0),
    (147, 6, 2000, 1000, ("wide", 10, 0), None, None, 0, 0),
    (140, 20, 2000, 1000, ("wide", 10, 1), None, None, 0, 0),
    (121, 36, 2001, 1000, ("wide", 10, 2), None, None, 0, 0),
    (100, 8, 2000, 1000, ("grouped_dma", 7, 0), None, None, 0, 0),
    (100, 8, 2001, 1000, ("grouped_vgpr", 7, 0), None, None, 0, 0),
    (170, 10, 2000, 1000, ("grouped_dma", 12, 1), None, None, 0, 0),
    (150, 30, 2000, 1000, ("grouped_vgpr", 12, 2), None, None, 0, _O),
]


@pytest.mark.parametrize("M,P,n,split,expect,ldx,ldy,xoff,yoff", INSTANCES)
def test_stats_record_of_every_instantiation(gpu_ctx, M, P, n, split, expect, ldx, ldy, xoff, yoff):
    _case(gpu_ctx, M, P, n, split, expect, ldx, ldy, xoff, yoff, seed=M + P)


# ---------------------------------------------------------------------------------------------------------------------------------
# row counts below and around one tile; splits at the edges; the grid clamp
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 65, 127, 129])
@pytest.mark.parametrize("M,P,fam_even,fam_odd", [(20, 8, "vgpr", "vgpr"), (50, 30, "dma8", "vgpr"), (128, 16, "wide", "wide"),
                                                  (100, 8, "grouped_dma", "grouped_vgpr")])
def test_stats_record_few_rows(gpu_ctx, n, M, P, fam_even, fam_odd):
    X, Y = _data(n, M, P, n)
    for split in sorted({0, n // 2, n}):
        fam, C, CY = kernel_for(M, P, n, split)
        assert fam == (fam_even if n % 2 == 0 else fam_odd), fam
        _check(_record(gpu_ctx, X, Y, split), X, Y, split, fam, C, CY)


@pytest.mark.parametrize("M,P,n,fam", [(20, 20, 3001, "vgpr"), (40, 20, 3000, "dma8"), (128, 16, 3000, "wide"),
                                       (170, 10, 3000, "grouped_dma")])
def test_stats_record_splits(gpu_ctx, M, P, n, fam):
    """the split at 0, at n, on a 128-row tile boundary and one either side, on a 64-row boundary, odd"""
    X, Y = _data(n, M, P, 5)
    rec0 = None
    for split in (0, n, 128, 127, 129, 1024, 1025, 1088, 1499):
        got = kernel_for(M, P, n, split)
        assert got[0] == fam, got
        rec = _record(gpu_ctx, X, Y, split)
        _check(rec, X, Y, split, *got)
        if rec0 is not None:
            assert np.array_equal(rec[2:18], rec0[2:18])            # the shift does not depend on the split
        rec0 = rec


@pytest.mark.parametrize("M,P,n,split,fam", [
    (5, 3, 66001, 66001, "vgpr"),             # k_gram, 8 waves: 256 work-groups from 65 400 rows in a partition
    (50, 10, 98305, 98305, "vgpr"),           # k_gram, 4 waves: 384 from 98 000
    (40, 20, 17000, 0, "dma8"),               # 128 from 16 300 (validation rows only)
    (128, 16, 17000, 17000, "wide"),
    (100, 8, 33001, 33001, "grouped_vgpr"),   # k_gram<6, 0, true>: 128 from 32 600
    (170, 10, 17000, 17000, "grouped_dma"),
])
def test_stats_record_at_the_grid_clamp(gpu_ctx, M, P, n, split, fam):
    got = kernel_for(M, P, n, split)
    assert got[0] == fam, got
    G, cap = work_groups(fam, got[1], n, split)
    assert G == cap, (G, cap)
    X, Y = _data(n, M, P, 9)
    _check(_record(gpu_ctx, X, Y, split), X, Y, split, *got)


def test_stats_record_of_no_rows(gpu_ctx):
    """n == 0: an all-zero record (every entry written)"""
    for M, P in ((5, 3), (50, 30), (128, 16), (100, 8), (170, 10)):
        X, Y = np.zeros((0, M), order="F"), np.zeros((0, P), order="F")
        rec = _record(gpu_ctx, X, Y, 0)
        assert np.all(rec == 0), (M, P, np.nonzero(rec != 0)[0][:5])


# ---------------------------------------------------------------------------------------------------------------------------------
# shards: row0, the global training count before / inside / after the shard; records about one shift add up
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,bounds", [(32, 16, (0, 2000, 4100, 6000)), (50, 30, (0, 2001, 4100, 6000)), (128, 16, (0, 3000, 6000)),
                                        (100, 8, (0, 1999, 6000)), (170, 10, (0, 2500, 3333, 6000))])
@pytest.mark.parametrize("ntrain", [0, 2500, 6000, 4100])
def test_stats_record_shards_add_up(gpu_ctx, M, P, bounds, ntrain):
    """shards of one set (each a view into the whole set: ld = N > n, base pointer row0 rows in) accumulated about the WHOLE
    set's shift, with row0 > 0 and the global training count before, inside and after a shard: every shard's record is exact,
    and their sum is the whole set's record entry by entry"""
    N = bounds[-1]
    X, Y = _data(N, M, P, 17)
    full = _record(gpu_ctx, X, Y, ntrain)
    fam, C, CY = kernel_for(M, P, N, ntrain)
    refs = _check(full, X, Y, ntrain, fam, C, CY)
    C16 = 16 * C
    shift = full[2:2 + C16]
    total = np.zeros_like(full)
    for a, b in zip(bounds[:-1], bounds[1:]):
        Xs, Ys = X[a:b], Y[a:b]
        split = min(max(ntrain - a, 0), b - a)
        sfam, sC, sCY = kernel_for(M, P, b - a, ntrain, N, N, 8 * a, 8 * a)
        # the shard through a view of the whole set's columns
        rec = _shard_record(gpu_ctx, X, Y, a, b, ntrain, shift)
        _check(rec, Xs, Ys, split, sfam, sC, sCY, check_shift=False)
        total[2 + C16:] += rec[2 + C16:]
        total[:2] += rec[:2]
    _, _, sums, G = _parts(full, C16)
    _, _, tsums, tG = _parts(total, C16)
    K = M + P
    for part in (0, 1):
        _, a_ref, G_ref = refs[part]
        assert np.all(np.abs(tsums[part][:K] - sums[part][:K]) <= TOL * a_ref.astype(np.float64))
        d = np.diag(G_ref).astype(np.float64)
        assert np.all(np.abs(tG[part] - G[part])[:K, :K] <= TOL * np.sqrt(np.outer(d, d)))
    assert np.array_equal(total[:2], full[:2])


def _shard_record(gpu_ctx, X, Y, a, b, ntrain, shift):
    """rows [a, b) of the whole set's device columns (leading dimension N, base pointers a rows in), row0 = a"""
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    N, M = X.shape
    P = Y.shape[1]
    tX, pX = _dev_cols(X, N, 0)
    tY, pY = _dev_cols(Y, N, 0)
    st = torch.full((L.abc_stats_len(M, P),), float("nan"), dtype=torch.float64, device="cuda:0")
    st[2:2 + len(shift)] = torch.from_numpy(shift.copy()).to("cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.check(L.abc_stats_accumulate_dev(gpu_ctx.handle, pX + 8 * a, pY + 8 * a, b - a, N, N, M, P, a, ntrain, st.data_ptr()))
    torch.cuda.synchronize()
    return st.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# strides and offsets: NaN gap rows, ldx != ldy; bit-identical to the contiguous call where the branch is the same
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,n", [(20, 20, 3000), (20, 20, 3001), (50, 30, 3000), (128, 16, 3000), (100, 8, 3000), (170, 10, 3001)])
@pytest.mark.parametrize("dx,dy,xoff,yoff", [(2, 64, 0, 0), (64, 2, 0, 0), (1, 2, 0, 0), (2, 1, 0, 0), (64, 65, 0, 0),
                                             (0, 0, _O, 0), (2, 64, 0, _O)])
def test_stats_record_strided_and_offset(gpu_ctx, M, P, n, dx, dy, xoff, yoff):
    X, Y = _data(n, M, P, 23)
    split = n // 2 + 1
    base = kernel_for(M, P, n, split)
    got = kernel_for(M, P, n, split, n + dx, n + dy, 8 * xoff, 8 * yoff)
    rec = _record(gpu_ctx, X, Y, split, n + dx, n + dy, xoff, yoff)
    _check(rec, X, Y, split, *got)
    if dx % 2 == 0 and dy % 2 == 0 and xoff == yoff == 0:       # the same alignment and leading-dimension parity as ld = n
        assert got == base
        assert np.array_equal(rec, _record(gpu_ctx, X, Y, split)), "a leading dimension of the same parity changed the record"


# ---------------------------------------------------------------------------------------------------------------------------------
# data: constant columns, a column far from zero, an unrepresentative pilot
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["constant", "far"])
@pytest.mark.parametrize("M,P,n,fam", [(20, 20, 3000, "vgpr"), (50, 30, 3000, "dma8"), (50, 30, 3001, "vgpr"), (128, 16, 3000, "wide"),
                                       (100, 8, 3001, "grouped_vgpr"), (170, 10, 3000, "grouped_dma")])
def test_stats_record_awkward_columns(gpu_ctx, kind, M, P, n, fam):
    X, Y, rec = _case(gpu_ctx, M, P, n, n // 2, (fam,) + kernel_for(M, P, n, n // 2)[1:], kind=kind, seed=31)
    if kind == "constant":
        C16 = 16 * ((M + P + 15) // 16)
        _, shift, sums, G = _parts(rec, C16)
        assert shift[1] == 3.25 and sums[0][1] == 0 and np.all(G[0][1, :] == 0) and np.all(G[1][:, 1] == 0)


@pytest.mark.parametrize("M,P,n,fam", [(20, 20, 5000, "vgpr"), (50, 30, 5000, "dma8"), (128, 16, 5001, "wide"),
                                       (170, 10, 5000, "grouped_dma")])
def test_stats_record_with_an_unrepresentative_pilot(gpu_ctx, M, P, n, fam):
    """the first 256 rows (the pilot the shift is taken from) 1e3 sigma away from the rest -- a grid-ordered first set: every
    V is then ~1e3 sigma, and the centred covariance G - s s'/rows cancels.  Bound on the centred covariance of a partition:
    |G - G*| <= 1e-13 sqrt(G_aa G_bb) (the record's) and |s_a s_b - s*_a s*_b| / rows <= 2e-13 sqrt(G_aa G_bb) (Cauchy-Schwarz:
    |s_a| <= sum |v_a| <= sqrt(rows G_aa)), plus the two roundings of the subtraction: 4e-13 sqrt(G_aa G_bb) in all.  Against the
    two-pass long double covariance; the test also states how much the pilot costs, sqrt(G_aa G_bb) / (rows sigma_a sigma_b)"""
    split = n // 2
    X, Y, rec = _case(gpu_ctx, M, P, n, split, (fam,) + kernel_for(M, P, n, split)[1:], kind="pilot", seed=41)
    K, C16 = M + P, 16 * ((M + P + 15) // 16)
    _, shift, sums, G = _parts(rec, C16)
    Z = np.hstack([X, Y])
    worst_amp = 0.0
    for part, (a, b) in enumerate(((0, split), (split, n))):
        rows = b - a
        s = sums[part][:K]
        cov = G[part][:K, :K] - np.outer(s, s) / rows
        Zl = Z[a:b].astype(np.longdouble)
        ref = _gram_ld((Zl - Zl.mean(axis=0)).astype(np.float64))    # (fp64 rounding of the centred values: 2 u relative)
        dG = np.diag(G[part])[:K]
        bound = 4e-13 * np.sqrt(np.outer(dG, dG))
        if not fam.startswith("grouped") and kernel_for(M, P, n, split)[2]:
            y0 = 16 * (kernel_for(M, P, n, split)[1] - kernel_for(M, P, n, split)[2])
            ref[y0:, y0:] = np.where(np.eye(K - y0, dtype=bool), ref[y0:, y0:], cov[y0:, y0:])   # skipped blocks: not compared
        err = np.abs(cov.astype(np.longdouble) - ref)
        assert np.all(err <= bound), (part, float((err / bound).max()))
        amp = np.sqrt(dG) / np.sqrt(np.diag(ref).astype(np.float64))
        worst_amp = max(worst_amp, float(amp.max()))
    assert worst_amp > 10, worst_amp          # the pilot really is unrepresentative
    print("unrepresentative pilot, %s: the record's scale is %.0f x the centred one" % (fam, worst_amp))


# ---------------------------------------------------------------------------------------------------------------------------------
# stage timing: the same record, and a bracket around every launch of every launch body
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,n,fam", [(32, 16, 1000, "vgpr"), (40, 20, 1000, "dma8"), (128, 16, 1000, "wide"),
                                       (100, 8, 1000, "grouped_dma"), (100, 8, 1001, "grouped_vgpr"), (170, 10, 1000, "grouped_dma")])
def test_stats_record_under_stage_timing(gpu_ctx, M, P, n, fam):
    """abc_timing_enable does not change a byte of the record, and the k_gram and stats_reduce stages are counted once per launch
    of the plan: once, on the grouped path once per pair of column groups (the smallest shapes that reach each launch body; the
    byte-limb kernel needs 200 000 rows: tests/test_gpu_parity.py::test_wide_gram_on_the_i8_matrix_pipe)"""
    split = n // 2
    p = plan(M, P, n, split)
    assert p["kernel"] == fam and p["launches"] == (1 if not fam.startswith("grouped") else p["pairs"]) >= 1, p
    X, Y = _data(n, M, P, 3)
    plain = _record(gpu_ctx, X, Y, split)
    gpu_ctx.timing_enable(True)
    try:
        gpu_ctx.timing_read(reset=True)
        timed = _record(gpu_ctx, X, Y, split)
        stages = gpu_ctx.timing_read(reset=True)
    finally:
        gpu_ctx.timing_enable(False)
    assert timed.tobytes() == plain.tobytes()
    assert stages["k_gram"][2] == p["launches"] and stages["stats_reduce"][2] == p["launches"], (stages["k_gram"], stages["stats_reduce"])
