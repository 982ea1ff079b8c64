"""ABC-GLM posterior of the batched ranking (abc_glm_rank_targets_dev, abc_glm_particle_ranking_pls_targets, abc_glm_weighted*):
every case of tests/_glm_cases.py through both batched entries and the generic entry against the NumPy reference of the header's
definition (tests/_glm_ref.py, in long double), on scores rebuilt from the fit's R, mean and sd.

Bars.  C, c0, sigma_s, T, mean, var and log_md within 1e-9 relative, the suite's bar for fp64 stages, taken per target and output
against the largest magnitude of the reference's array (a mean has no zero of its own: an entry near 0 is measured against its
neighbours).  The density within the marginal density's bar, |f_dev - f_ref| <= 1e-6 f_ref + 1e-290 max f_ref, against a
long-double evaluation at the device's own T, peaks, c and grid; lo_x and step bit for bit from the device's own peaks and T; the
mode is the first grid point at which the device's own density is largest.  Bit identity: on a repeat, alone against in a batch,
device against host entry, with against without dens / peaks, idx and dist against abc_rank_targets_dev."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _density_ref as D
import _glm_cases as GC
import _glm_ref as R
import _loclinear_ref as LL
import _pls_ref as PR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from abcsmc_amd._lib import GLM_OUTPUTS as ALL            # (the file fails at collection where the entries do not exist)
MODEL = ("C", "c0", "sigma_s", "T", "mean", "var", "log_md")


def fit(ctx, X, Y, A, f=0.5):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    N, M = X.shape
    P = Y.shape[1]
    Xd, Yd = device.colmajor(X, DEV), device.colmajor(Y, DEV)
    stats = torch.empty(L.abc_stats_len(M, P), dtype=torch.float64, device=DEV)
    model = torch.empty(L.abc_model_len(M, P, A), dtype=torch.float64, device=DEV)
    obs = torch.zeros(M, dtype=torch.float64, device=DEV)
    ntr = int(np.floor(f * N + 0.5))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(L.abc_stats_shift_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, stats.data_ptr()))
    ctx.check(L.abc_stats_accumulate_dev(ctx.handle, Xd.data_ptr(), Yd.data_ptr(), N, N, N, M, P, 0, ntr, stats.data_ptr()))
    ctx.check(L.abc_pls_model_dev(ctx.handle, stats.data_ptr(), obs.data_ptr(), M, P, A, 0, model.data_ptr()))
    torch.cuda.synchronize()
    return dict(Xd=Xd, Yd=Yd, model=model, A=A, M=M, P=P)


def to_np(r):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def same(a, b):
    """the same bits up to the payload of a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def weighted_dev(ctx, th, st, ob, w, G=64, cut=3.0, bw=None, outputs=ALL):
    """abc_glm_weighted_dev on device copies; returns host arrays"""
    import torch
    from abcsmc_amd import _lib
    K, P = th.shape
    n = st.shape[1]
    t = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T), device=DEV)
    thd, std, obd = t(th), t(st), t(ob)
    wd = None if w is None else t(w)
    bwd = None if bw is None else t(bw)
    sh = _lib.glm_shapes((), K, P, n, G)
    r = {k: (torch.empty(sh[k], dtype=torch.int32 if k == "status" else torch.float64, device=DEV) if k in outputs else None) for k in ALL}
    p = lambda v: v.data_ptr() if v is not None else None
    d = _lib.Glm(G, cut, 1.0, p(bwd), *[p(r[k]) for k in ALL])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(_lib.lib().abc_glm_weighted_dev(C.byref(d), ctx.handle, thd.data_ptr(), K, std.data_ptr(), K, K, P, n, obd.data_ptr(), p(wd)))
    return to_np(r)


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def run_dev(ctx, F, T, c, ex, om, bw, nc=None, outputs=ALL, G=None):
    import torch
    from abcsmc_amd import device
    model = F["model"]
    if nc is not None:
        model = model.clone()
        model[0] = float(nc)
    e = torch.tensor(ex, dtype=torch.int64) if ex is not None else None
    with (ctx.row_weights(om) if om is not None else contextlib.nullcontext()):
        return to_np(device.rank_targets_glm(F["Xd"], model, F["A"], device.colmajor(T, DEV), c["K"], F["Yd"], G=G or c["G"], bw=bw,
                                             exclude=e, dist=True, outputs=outputs, ctx=ctx))


def rel(a, b):
    b = np.asarray(b, dtype=LD)
    return float(np.abs(np.asarray(a).astype(LD) - b).max() / np.abs(b).max())


def check_density(r, cut, G, every=1):
    """one target's dens, lo_x, step, mode and mode_dens against its own T, peaks and c (dens at every `every`-th grid point)"""
    P = r["T"].shape[0]
    keep = r["c"] > 0
    worst = 0.0
    for j in range(P):
        sd = np.sqrt(r["T"][j, j])
        tj = r["peaks"][np.isfinite(r["peaks"][:, j]), j]
        lo_x, step = D.grid(tj.min(), tj.max(), sd, cut, G)
        assert lo_x == r["lo_x"][j] and step == r["step"][j], (j, lo_x, r["lo_x"][j], step, r["step"][j])
        xg = D.grid_points(lo_x, step, G)
        f = R.mixture_density(xg[::every], r["peaks"][keep, j], r["c"][keep], r["T"][j, j])
        err = np.abs(r["dens"][j][::every].astype(LD) - f)
        bound = LD(1e-6) * f + LD(1e-290) * f.max()
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (j, float((err / bound).max()))
        g = int(np.argmax(r["dens"][j]))
        assert r["mode"][j] == xg[g] and r["mode_dens"][j] == r["dens"][j, g], j
    return worst


def check_target(name, got, theta, S_rows, o, w, c, bw):
    ref = R.glm(theta, S_rows, o, w, G=2, cut=3.0, bw=bw, dtype=LD)
    assert int(got["status"]) == 0 and ref["status"] == 0, name
    for k in MODEL:
        e = rel(got[k], ref[k])
        print("%s %-8s %.2e" % (name, k, e))
        assert e <= 1e-9, (name, k, e)
    assert rel(got["ess"], ref["ess"]) <= 1e-9 and rel(got["c"], ref["c"]) <= 1e-9
    counted = np.ones(theta.shape[0], bool) if w is None else w > 0
    assert np.all(np.isnan(got["peaks"][~counted])) and np.all(got["c"][~counted] == 0)
    assert rel(got["peaks"][counted], ref["peaks"][counted]) <= 1e-9
    print("%s density: worst error %.3f of its bound" % (name, check_density(got, 3.0, c["G"])))


@pytest.mark.parametrize("row", GC.CASES, ids=[r[0] for r in GC.CASES])
def test_case_against_the_reference(ctx, row):
    from abcsmc_amd import device, glm
    c = GC.case(row)
    X, Y, T, ex, om, bw = GC.inputs(c)
    K, P, B, nc = c["K"], c["P"], c["B"], c["nc"]
    F = fit(ctx, X, Y, nc)
    m = PR.unpack_model(F["model"].cpu().numpy(), c["M"], P, nc)
    nat = int(m["hdr"][0])
    assert 1 <= nat <= nc
    # device entry at the fit's own ncomp against the host entry: the same bits; idx and dist those of the plain ranking
    dn = run_dev(ctx, F, T, c, ex, om, bw)
    host = glm.particle_ranking_PLS_targets_glm(X, Y, T, 0.5, K, G=c["G"], bw=bw, exclude=ex, max_comp=nc, rule=0, ctx=ctx,
                                                row_weights=om, outputs=ALL)
    assert host["ncomp"] == nat == dn["ncomp"]
    assert np.array_equal(host["idx"].astype(np.int64), dn["idx"]) and same(host["dist"], dn["dist"])
    for k in ALL:
        assert same(host[k], dn[k]), k
    import torch
    Td = torch.empty((c["M"], B), dtype=torch.float64, device=DEV)         # (unit stride along the targets, also at B = 1)
    Td.copy_(torch.tensor(T, device=DEV).T)
    pidx, pdist, _ = device.rank_targets(F["Xd"], F["model"], nc, Td, K, F["Yd"],
                                         exclude=torch.tensor(ex, dtype=torch.int64) if ex is not None else None, dist=True, ctx=ctx)
    plain = to_np(dict(idx=pidx, dist=pdist))
    assert np.array_equal(plain["idx"], dn["idx"]) and same(plain["dist"], dn["dist"])
    # at the case's ncomp: against the reference, target by target, with the generic entry on the same rows
    r = dn if nat == nc else run_dev(ctx, F, T, c, ex, om, bw, nc=nc)
    assert r["ncomp"] == nc and r["C"].shape == (B, nc, P)
    S = LL.scores(X, m["mean"][:c["M"]], m["sd"][:c["M"]], m["R"], nc)
    O = LL.scores(T, m["mean"][:c["M"]], m["sd"][:c["M"]], m["R"], nc)
    for b in range(B):
        ix = r["idx"][b]
        w = None if om is None else om[ix]
        bwb = None if bw is None else bw[b]
        check_target("%s[%d]" % (c["name"], b), {k: r[k][b] for k in ALL}, Y[ix], S[ix], O[b], w, c, bwb)
        if b < 2:
            g = glm.weighted_glm(Y[ix], S[ix], O[b], w, G=c["G"], bw=bwb, ctx=ctx, outputs=ALL)
            check_target("%s[%d] generic" % (c["name"], b), g, Y[ix], S[ix], O[b], w, c, bwb)
            gd = weighted_dev(ctx, Y[ix], S[ix], O[b], w, G=c["G"], bw=bwb)
            for k in ALL:
                assert same(g[k], gd[k]), k
    # the same bits on a repeat, alone, and whatever is asked for
    again = run_dev(ctx, F, T, c, ex, om, bw, nc=nc)
    for k in ALL + ("idx", "dist"):
        assert same(again[k], r[k]), k
    for b in sorted({0, B - 1}):
        alone = run_dev(ctx, F, T[b:b + 1], c, None if ex is None else ex[b:b + 1], om, None if bw is None else bw[b:b + 1], nc=nc)
        for k in ALL:
            assert same(alone[k][0], r[k][b]), (k, b)
    few = ("lo_x", "step", "mode", "mode_dens", "mean", "var", "ess", "log_md", "status")
    less = run_dev(ctx, F, T, c, ex, om, bw, nc=nc, outputs=few)
    for k in few:
        assert same(less[k], r[k]), k
    assert less["dens"] is None and less["peaks"] is None


def test_grid_beyond_one_chunk_and_many_chunks_of_rows(ctx):
    """G = 1100 (three chunks of grid points, the candidates' pass) at K = 20000 (64 chunks of rows): the generic entry against
    the reference and its density against its own peaks"""
    from abcsmc_amd import glm
    rng = np.random.default_rng(5)
    K, P, n = 20000, 2, 2
    th = rng.normal(size=(K, P)) * [0.7, 1.6] + [1.0, -2.0]
    st = th @ rng.normal(size=(P, n)) + 0.5 * rng.normal(size=(K, n))
    ob = st[0] + 0.2
    w = rng.uniform(0.1, 1.0, size=K)
    g = glm.weighted_glm(th, st, ob, w, G=1100, ctx=ctx, outputs=ALL)
    ref = R.glm(th, st, ob, w, G=2, dtype=LD)
    for k in MODEL:
        assert rel(g[k], ref[k]) <= 1e-9, (k, rel(g[k], ref[k]))
    print("worst density error %.3f of its bound" % check_density(g, 3.0, 1100, every=5))
    few = glm.weighted_glm(th, st, ob, w, G=1100, ctx=ctx, outputs=("mode", "mode_dens"))
    assert same(few["mode"], g["mode"]) and same(few["mode_dens"], g["mode_dens"])


def test_uncorrelated_design_is_the_kernel_density(ctx):
    """M_thx = 0: C = 0, c^_e = w_e / W, the peaks are the rows and T_jj = h_j^2, so dens is abc_weighted_density's at the same bw"""
    from abcsmc_amd import abcutil, glm
    from test_glm_cpu import paired_design
    th, x, w = paired_design(half=40)
    h = np.array([0.3, 0.45])
    g = glm.weighted_glm(th, x, [0.25, -0.5], w, G=257, bw=h, ctx=ctx, outputs=ALL)
    assert g["status"] == 0 and np.abs(g["C"]).max() < 1e-15
    kde = abcutil.weighted_density(th, w, G=257, bw=h, ctx=ctx)
    f = kde["dens"].astype(LD)
    for j in range(2):
        assert np.all(np.abs(g["dens"][j].astype(LD) - f[j]) <= LD(1e-6) * f[j] + LD(1e-290) * f[j].max()), j
    xbar = (w[:, None] * x).sum(axis=0) / w.sum()
    d = np.array([0.25, -0.5]) - xbar
    ref = -0.5 * (d @ np.linalg.solve(g["sigma_s"], d)) - 0.5 * (2 * np.log(2 * np.pi) + np.log(np.linalg.det(g["sigma_s"])))
    assert abs(g["log_md"] - ref) <= 1e-9 * abs(ref)


def test_status_bits(ctx):
    """a duplicated parameter column: bit 0; K = P + 1: bit 1; one NaN row: bit 2; every output of that target NaN, and the
    other targets of the batch untouched"""
    from abcsmc_amd import device, glm
    c = dict(K=40, G=9)
    X, Y = GC.table(800, 5, 3, 21)
    T = X[[3, 30]] + 0.05
    F = fit(ctx, X, Y, 2)
    good = run_dev(ctx, F, T, c, None, None, None)
    assert np.array_equal(good["status"], [0, 0])

    def all_nan(r, b):
        return all(np.all(np.isnan(r[k][b])) for k in ALL if k != "status")

    Yd = Y.copy()
    Yd[:, 2] = Yd[:, 0]
    Fd = dict(fit(ctx, X, Y, 2), Yd=device.colmajor(Yd, DEV))
    r = run_dev(ctx, Fd, T, c, None, None, None)
    assert np.array_equal(r["status"], [1, 1]) and all_nan(r, 0) and all_nan(r, 1)
    r = run_dev(ctx, F, T, dict(K=4, G=9), None, None, None)
    assert np.array_equal(r["status"], [2, 2]) and all_nan(r, 0)
    Yn = Y.copy()
    row = int(good["idx"][0, 7])
    assert row not in good["idx"][1]
    Yn[row, 1] = np.nan
    Fn = dict(F, Yd=device.colmajor(Yn, DEV))
    r = run_dev(ctx, Fn, T, c, None, None, None)
    assert np.array_equal(r["status"], [4, 0]) and all_nan(r, 0)
    for k in ALL:
        assert same(r[k][1], good[k][1]), k
    # the documented deviation: the bandwidth rule reads every entry, so a non-finite theta in a row of weight 0 is bit 2 as well
    om = np.ones(800)
    om[row] = 0.0
    r = run_dev(ctx, Fn, T, c, None, om, None)
    assert np.array_equal(r["status"], [4, 0]) and all_nan(r, 0)
    # no counted row at all (every retained row of target 0 weighs 0): n_eff is NaN, bit 1
    om = np.ones(800)
    om[good["idx"][0]] = 0.0
    r = run_dev(ctx, F, T, c, None, om, None)
    assert r["status"][0] == 2 and all_nan(r, 0) and r["status"][1] == 0
    th, st = Y[:30], X[:30, :2]
    bad = st.copy()
    bad[4, 1] = np.inf
    g = glm.weighted_glm(th, bad, st[0], None, G=5, ctx=ctx, outputs=ALL)
    assert g["status"] == 4 and all(np.all(np.isnan(g[k])) for k in ALL if k != "status")
    g = glm.weighted_glm(th[:4], st[:4], st[0], None, G=5, ctx=ctx, outputs=ALL)
    assert g["status"] == 2


def test_refused_arguments(ctx):
    import torch
    from abcsmc_amd import _lib, device
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -4
    X, Y = GC.table(400, 5, 3, 22)
    F = fit(ctx, X, Y, 2)
    T = device.colmajor(X[:2], DEV)
    buf = torch.empty(4096, dtype=torch.float64, device=DEV)
    idx = torch.empty(2 * 20, dtype=torch.int64, device=DEV)

    def desc(G=16, cut=3.0, bw_scale=1.0, out=True):
        d = _lib.Glm(G, cut, bw_scale, None, *([None] * len(ALL)))
        if out:
            d.mean = buf.data_ptr()
        return d

    def dev(d, P=3, A=2, model=None, Yd=None, M=5):
        model = F["model"] if model is None else model
        Yd = F["Yd"] if Yd is None else Yd
        return L.abc_glm_rank_targets_dev(C.byref(d) if d is not None else None, ctx.handle, F["Xd"].data_ptr(), 400, Yd.data_ptr(), 400, 400,
                                          M, P, model.data_ptr(), A, T.data_ptr(), 2, 2, None, 20, idx.data_ptr(), None)

    th = torch.zeros(40 * 33, dtype=torch.float64, device=DEV)

    def gen(d, P=3, n=2):
        return L.abc_glm_weighted_dev(C.byref(d), ctx.handle, th.data_ptr(), 40, th.data_ptr(), 40, 40, P, n, th.data_ptr(), None)

    def code(rc):
        msg = L.abc_last_error(ctx.handle)
        assert rc == 0 or (msg and len(msg) > 10), rc                 # (every refusal comes with a message)
        return rc

    assert dev(desc()) == 0
    assert code(dev(None)) == INVALID
    for kw in (dict(G=1), dict(G=4097), dict(cut=-1.0), dict(cut=float("nan")), dict(cut=float("inf")), dict(bw_scale=0.0),
               dict(bw_scale=float("inf")), dict(out=False)):
        assert code(dev(desc(**kw))) == INVALID, kw
        assert code(gen(desc(**kw))) == INVALID, kw
    assert code(dev(desc(), A=65)) == INVALID
    Y33 = torch.zeros(33 * 400, dtype=torch.float64, device=DEV)
    assert code(dev(desc(), P=33, Yd=Y33)) == INVALID
    assert code(gen(desc(), P=33)) == INVALID and code(gen(desc(), P=0)) == INVALID
    assert code(gen(desc(), n=33)) == INVALID and code(gen(desc(), n=0)) == INVALID
    big = torch.zeros(L.abc_model_len(5, 3, 40), dtype=torch.float64, device=DEV)
    big[0] = 33.0
    assert code(dev(desc(), A=40, model=big)) == INVALID                 # ncomp = 33
    with ctx.param_transf(*_lib.transf_arrays(["log", "none", "none"], None, None)):
        assert code(dev(desc())) == UNSUPPORTED and code(gen(desc())) == UNSUPPORTED
    with ctx.adjust_hcorr(True):
        assert code(dev(desc())) == UNSUPPORTED and code(gen(desc())) == UNSUPPORTED
    with ctx.adjust_ridge([0.1]):
        assert code(dev(desc())) == UNSUPPORTED and code(gen(desc())) == UNSUPPORTED
    assert dev(desc()) == 0 and gen(desc()) == 0
    torch.cuda.synchronize()


def test_entries_keep_to_their_reservation_fresh_and_poisoned(tmp_path):
    """tests/_glm_worker.py as the environment is and under ABC_WS_POISON=ff: the four entries on a fresh context and on one whose
    arena a larger call has grown; abc_ws_info's peak never exceeds what the entry asked for and reserved, and every output has
    the same bytes in all four runs"""
    runs = {}
    for child in ("plain", "poison"):
        out = str(tmp_path / (child + ".npz"))
        env = dict(os.environ)
        env.pop("ABC_WS_POISON", None)
        if child == "poison":
            env["ABC_WS_POISON"] = "ff"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_glm_worker.py"), out], capture_output=True, text=True,
                           timeout=120, env=env, cwd=ROOT)
        assert p.returncode == 0, (child, p.stdout[-2000:], p.stderr[-3000:])
        with np.load(out) as z:
            runs[child] = {k: z[k] for k in z.files}
    ref = runs["plain"]
    keys = sorted(ref)
    assert len([k for k in keys if k.endswith("|info")]) == 8 and sorted(runs["poison"]) == keys
    for child in runs:
        for k in keys:
            mode, name, field = k.split("|")
            v = runs[child][k]
            if field == "info":
                reserved, asked, peak = (int(x) for x in v)
                print(child, mode, name, "reserved %d asked %d peak %d" % (reserved, asked, peak))
                assert peak <= asked <= reserved, (child, k, v)
            else:
                a = ref["fresh|%s|%s" % (name, field)]
                assert a.dtype == v.dtype and a.shape == v.shape and a.tobytes() == v.tobytes(), (child, k)
