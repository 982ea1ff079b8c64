"""Exact quantiles and CDF of the ABC-GLM marginals (abc_glm_rank_targets_summary_dev, abc_glm_particle_ranking_pls_targets_summary,
abc_glm_weighted_summary*) against tests/_glm_summary_ref.py.

Bars.  F_ref and f_ref are built from the device's own peaks, c and T of the same call, so the model's rounding does not enter:
    |F_ref(quant) - q|   <= (K + 8) 2^-52 + 2 f_ref(quant) spacing(quant)
    |cdf - F_ref(truth)| <= (K + 8) 2^-52
K the counted rows: the worst-case rounding of a K-term fp64 sum of values in [0, 1] whose weights add to 1, and what one spacing of
x is worth in F.  Plain-fp64 bisection on the CPU reaches 0.41 of the bar at worst, a Phi of 1e-7 accuracy does not pass.  Every
figure is printed before it is asserted."""
import contextlib
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _glm_cases as GC
import _glm_ref as R
import _glm_summary_ref as S
import _loclinear_ref as LL
import _pls_ref as PR
import test_gpu_glm as TG

pytestmark = pytest.mark.gpu

from abcsmc_amd._lib import SIGNATURES
assert "abc_glm_weighted_summary_dev" in SIGNATURES            # (the file fails at collection where the entries do not exist)

DEV = TG.DEV
ROOT = TG.ROOT
ALL = TG.ALL
same = TG.same
LEVELS = (1e-6, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0 - 1e-6)
# 64 levels: repeats, unsorted, from 1e-9 to 1 - 1e-9
LEVELS64 = tuple(np.random.default_rng(64).permutation(np.concatenate(
    [[1e-9, 1.0 - 1e-9, 0.5, 0.5, 0.025, 0.025], np.linspace(0.001, 0.999, 50), 10.0 ** -np.arange(2.0, 10.0)])))
assert len(LEVELS64) == 64


@pytest.fixture(scope="module")
def ctx():
    from abcsmc_amd import _lib
    return _lib.default_context(0)


def sample(K, P, n, seed, loc=0.0, spread=1.0, bimodal=False, weights=None):
    """theta (K, P) about loc, statistics that say little about it (the peaks stay near the rows), obs, w and the peak widths bw"""
    rng = np.random.default_rng(seed)
    if bimodal:     # rows in +- pairs on a grid of 1/8 with the same statistics and weight (test_glm_cpu.paired_design): M_thx = 0, the
        # peaks are the rows and c^ is symmetric, two groups within [8, 10] and [-10, -8]: the median falls in the empty gap
        h = K // 2
        th = 9.0 + rng.integers(-8, 9, size=(h, P)) / 8.0
        st = rng.integers(-16, 17, size=(h, n)) / 8.0
        w = rng.integers(1, 5, size=h).astype(np.float64)
        return np.concatenate([th, -th]), np.concatenate([st, st]), np.array([0.25, -0.5])[:n], np.concatenate([w, w]), np.full(P, 0.3)
    th = rng.normal(size=(K, P))
    st = 0.2 * th[:, :1] + rng.normal(size=(K, n))
    th = loc + spread * th
    w = None
    if weights == "zeros":
        w = rng.uniform(0.1, 1.0, size=K)
        w[::7] = 0.0
    elif weights == "wide":                                 # 1e-12 .. 1
        w = 10.0 ** rng.uniform(-12.0, 0.0, size=K)
        w[0], w[-1] = 1e-12, 1.0
    return th, st, st[K // 2] + 0.1, w, np.full(P, 0.3 * spread)


def generic(ctx, th, st, ob, w, bw, probs=None, truth=None, outputs=("peaks", "c", "T", "status"), dev=False, G=16):
    """abc_glm_weighted_summary (host arrays) or abc_glm_weighted_summary_dev (device copies); host arrays back"""
    from abcsmc_amd import _lib, glm
    if not dev:
        return glm.weighted_glm(th, st, ob, w, G=G, bw=bw, ctx=ctx, outputs=outputs, probs=probs, truth=truth)
    import torch
    K, P = th.shape
    n = st.shape[1]
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T), device=DEV)
    thd, std, obd, wd, bwd, trd = t(th), t(st), t(ob), t(w), t(bw), t(truth)
    sh = _lib.glm_shapes((), K, P, n, G)
    r = {k: (torch.empty(sh[k], dtype=torch.int32 if k == "status" else torch.float64, device=DEV) if k in outputs else None) for k in ALL}
    pr = None if probs is None else np.ascontiguousarray(np.asarray(probs, dtype=np.float64))
    r["quant"] = None if pr is None else torch.empty((pr.size, P), dtype=torch.float64, device=DEV)
    r["cdf"] = None if truth is None else torch.empty(P, dtype=torch.float64, device=DEV)
    p = lambda v: v.data_ptr() if v is not None else None
    d = _lib.Glm(G, 3.0, 1.0, p(bwd), *[p(r[k]) for k in ALL])
    sm = _lib.Summary(None if pr is None else pr.ctypes.data, 0 if pr is None else pr.size, p(trd), p(r["quant"]), p(r["cdf"]))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(_lib.lib().abc_glm_weighted_summary_dev(C.byref(d), C.byref(sm), ctx.handle, thd.data_ptr(), K, std.data_ptr(), K, K, P, n,
                                                      obd.data_ptr(), p(wd)))
    return TG.to_np(r)


def check_outputs(name, r, probs=None, truth=None):
    """quant and cdf of one target against F_ref / f_ref of its own peaks, c and T; returns the worst share of the bars"""
    P = r["T"].shape[0]
    worst_q = worst_c = 0.0
    for j in range(P):
        t, c = S.counted(r["peaks"][:, j], r["c"])
        sigma = math.sqrt(r["T"][j, j])
        if probs is not None:
            for i, q in enumerate(probs):
                x = float(r["quant"][i, j])
                assert math.isfinite(x), (name, j, q)
                res = abs(S.F_ref(x, t, c, sigma) - q) / S.quant_bound(x, t, c, sigma)
                worst_q = max(worst_q, res)
                assert res <= 1.0, (name, j, q, x, res)
        if truth is not None:
            x, got = float(truth[j]), float(r["cdf"][j])
            if math.isnan(x):
                assert math.isnan(got), (name, j)
            elif math.isinf(x):
                assert got == (1.0 if x > 0 else 0.0), (name, j, got)
            else:
                res = abs(got - S.F_ref(x, t, c, sigma)) / S.cdf_bound(t)
                worst_c = max(worst_c, res)
                assert res <= 1.0, (name, j, x, got, res)
    print("%-22s K %5d  quant %.3f of its bar, cdf %.3f of its bar" % (name, len(t), worst_q, worst_c))
    return worst_q, worst_c


#         name              K     P   n   probs      options
CASES = [("k3_smallest",    3,    1,  1,  LEVELS,    dict()),
         ("k37_nq64",       37,   2,  2,  LEVELS64,  dict(weights="zeros")),
         ("k1024_nq1",      1024, 1,  1,  (0.3,),    dict()),
         ("k1025_wide",     1025, 1,  1,  LEVELS,    dict(weights="wide")),
         ("k5000",          5000, 2,  1,  LEVELS,    dict(weights="zeros")),
         ("p32_n32",        100,  32, 32, (0.025, 0.5, 0.975), dict()),
         ("bimodal_gap",    400,  1,  2,  (0.5, 0.25, 0.4999, 0.75), dict(bimodal=True)),
         ("far_1e6",        257,  2,  1,  LEVELS,    dict(loc=1e6, spread=1e-3))]


@pytest.mark.parametrize("row", CASES, ids=[r[0] for r in CASES])
def test_generic_entry_against_the_reference(ctx, row):
    name, K, P, n, probs, opt = row
    th, st, ob, w, bw = sample(K, P, n, 100 + K + P, **opt)
    base = generic(ctx, th, st, ob, w, bw, probs=probs)
    assert base["status"] == 0 and base["cdf"] is None and base["quant"].shape == (len(probs), P)
    peaks = base["peaks"]
    k = int(np.flatnonzero(np.isfinite(peaks[:, 0]))[0])
    sd = np.sqrt(np.diag(base["T"]))
    # the truth, one call each: one of the peaks, a far-out value, +-inf, NaN, and a value in the lower tail
    kinds = [peaks[k], np.nanmax(peaks, axis=0) + 30.0 * sd, np.full(P, np.inf), np.full(P, -np.inf), np.full(P, np.nan),
             np.nanmin(peaks, axis=0) - 3.0 * sd]
    for i, tr in enumerate(kinds):
        r = generic(ctx, th, st, ob, w, bw, probs=probs if i == 0 else None, truth=tr)
        assert same(r["peaks"], peaks) and same(r["c"], base["c"])
        if i == 0:
            assert same(r["quant"], base["quant"])           # (with and without cdf beside it)
        check_outputs("%s truth %d" % (name, i), r, probs if i == 0 else None, tr)
    if name == "bimodal_gap":
        med = base["quant"][0, 0]
        print("the median of the two groups %.17g, sd %.3g" % (med, sd[0]))
        assert peaks[peaks[:, 0] < 0, 0].max() + 5 * sd[0] < med < peaks[peaks[:, 0] > 0, 0].min() - 5 * sd[0], med
    # the device form of the generic entry: the same bits
    d = generic(ctx, th, st, ob, w, bw, probs=probs, truth=kinds[0], dev=True)
    h = generic(ctx, th, st, ob, w, bw, probs=probs, truth=kinds[0])
    for key in ("quant", "cdf", "peaks", "c", "T"):
        assert same(d[key], h[key]), key


def test_one_row_cannot_be_fitted(ctx):
    """K = 1: n_eff = 1 <= P + 1, status bit 1, and every quant and cdf entry is NaN"""
    r = generic(ctx, np.array([[0.5]]), np.array([[1.0]]), [1.0], None, [0.3], probs=LEVELS, truth=[0.5], outputs=("status",))
    assert r["status"] == 2 and np.all(np.isnan(r["quant"])) and np.all(np.isnan(r["cdf"]))


def table(N=400, M=6, P=3, seed=31):
    return GC.table(N, M, P, seed)


def run_dev(ctx, F, T, K, om=None, probs=None, truth=None, outputs=ALL, G=16, model=None):
    import torch
    from abcsmc_amd import device
    tr = None if truth is None else torch.tensor(np.ascontiguousarray(truth), device=DEV)
    with (ctx.row_weights(om) if om is not None else contextlib.nullcontext()):
        return TG.to_np(device.rank_targets_glm(F["Xd"], F["model"] if model is None else model, F["A"], device.colmajor(T, DEV), K, F["Yd"],
                                                G=G, dist=True, outputs=outputs, ctx=ctx, probs=probs, truth=tr))


@pytest.mark.parametrize("weights", [False, True], ids=["equal", "row_weights"])
def test_batched_entry_against_the_generic_entry(ctx, weights):
    """N = 400, M = 6, P = 3, B = 5, K = 40: every target against its own peaks (the bars above) and against the generic entry fed
    that target's gathered rows with NumPy scores (the scores differ by rounding, so 1e-9 of the sample's spread, the suite's bar
    for fp64 stages, and 1e-9 for the CDF)"""
    from abcsmc_amd import glm
    X, Y = table()
    B, K, P = 5, 40, 3
    T = X[[3, 77, 150, 222, 399]] + 0.05
    om = None
    if weights:
        om = np.random.default_rng(8).uniform(0.1, 1.0, size=400)
        om[::7] = 0.0
    truth = Y[[3, 77, 150, 222, 399]].copy()
    truth[1, 0], truth[2, 1], truth[3, 2] = np.inf, -np.inf, np.nan
    host = glm.particle_ranking_PLS_targets_glm(X, Y, T, 0.5, K, G=16, max_comp=2, rule=0, ctx=ctx, row_weights=om, outputs=ALL,
                                                probs=LEVELS, truth=truth)
    assert np.array_equal(host["status"], np.zeros(B)) and host["quant"].shape == (B, len(LEVELS), P) and host["cdf"].shape == (B, P)
    F = TG.fit(ctx, X, Y, 2)
    dv = run_dev(ctx, F, T, K, om, LEVELS, truth)
    assert dv["ncomp"] == host["ncomp"]
    for k in ALL + ("quant", "cdf"):
        assert same(host[k], dv[k]), k                       # device entry against host entry: the same bits
    nc = host["ncomp"]
    m = PR.unpack_model(F["model"].cpu().numpy(), 6, P, 2)
    Sx = LL.scores(X, m["mean"][:6], m["sd"][:6], m["R"], nc)
    O = LL.scores(T, m["mean"][:6], m["sd"][:6], m["R"], nc)
    for b in range(B):
        r = {k: host[k][b] for k in ALL + ("quant", "cdf")}
        check_outputs("batched[%d]" % b, r, LEVELS, truth[b])
        ix = host["idx"][b].astype(np.int64)
        g = glm.weighted_glm(Y[ix], Sx[ix], O[b], None if om is None else om[ix], G=16, ctx=ctx, outputs=("peaks", "T", "c", "status"),
                             probs=LEVELS, truth=truth[b])
        spread = np.nanmax(r["peaks"], axis=0) - np.nanmin(r["peaks"], axis=0) + np.sqrt(np.diag(r["T"]))
        err = np.abs(g["quant"] - r["quant"]) / spread
        print("batched[%d] against generic: quant %.2e of the spread" % (b, err.max()))
        assert err.max() <= 1e-9
        fin = np.isfinite(truth[b])
        assert np.abs(g["cdf"][fin] - r["cdf"][fin]).max() <= 1e-9 and same(g["cdf"][~fin], r["cdf"][~fin])


def test_bit_identity_and_the_glm_outputs_of_the_older_entry(ctx):
    from abcsmc_amd import device, glm
    X, Y = table(seed=32)
    K = 40
    rows = [3, 77, 150, 222, 301, 350, 399]
    T = X[rows] + 0.05
    truth = Y[rows]
    F = TG.fit(ctx, X, Y, 2)
    full = run_dev(ctx, F, T, K, None, LEVELS64, truth)
    assert np.array_equal(full["status"], np.zeros(7))
    again = run_dev(ctx, F, T, K, None, LEVELS64, truth)
    for k in ALL + ("quant", "cdf", "idx", "dist"):
        assert same(full[k], again[k]), k                    # a repeat
    for b in (0, 6):                                         # alone against in a batch of 7
        alone = run_dev(ctx, F, T[b:b + 1], K, None, LEVELS64, truth[b:b + 1])
        for k in ALL + ("quant", "cdf"):
            assert same(alone[k][0], full[k][b]), (k, b)
    bare = run_dev(ctx, F, T, K, None, LEVELS64, truth, outputs=())      # without dens / peaks or any other output of glm
    assert same(bare["quant"], full["quant"]) and same(bare["cdf"], full["cdf"]) and bare["dens"] is None and bare["peaks"] is None
    for i in (0, 17, 63):                                    # a level solved alone against among 63 others
        one = run_dev(ctx, F, T, K, None, (LEVELS64[i],), None, outputs=())
        assert one["cdf"] is None and same(one["quant"][:, 0], full["quant"][:, i]), i
    only_cdf = run_dev(ctx, F, T, K, None, None, truth, outputs=())
    assert only_cdf["quant"] is None and same(only_cdf["cdf"], full["cdf"])
    # the glm outputs of the new entry are those of the entry it extends
    old = TG.to_np(device.rank_targets_glm(F["Xd"], F["model"], F["A"], device.colmajor(T, DEV), K, F["Yd"], G=16, dist=True, outputs=ALL,
                                           ctx=ctx))
    for k in ALL + ("idx", "dist"):
        assert same(old[k], full[k]), k
    hold = glm.particle_ranking_PLS_targets_glm(X, Y, T, 0.5, K, G=16, max_comp=2, rule=0, ctx=ctx, outputs=ALL)
    hnew = glm.particle_ranking_PLS_targets_glm(X, Y, T, 0.5, K, G=16, max_comp=2, rule=0, ctx=ctx, outputs=ALL, probs=(0.5,))
    assert sorted(hnew) == sorted(list(hold) + ["quant", "cdf"]) and hnew["cdf"] is None
    for k in hold:
        assert same(hold[k], hnew[k]), k
    th, st, ob, w, bw = sample(300, 2, 2, 9, weights="zeros")
    gold = glm.weighted_glm(th, st, ob, w, G=600, ctx=ctx, outputs=ALL)
    gnew = glm.weighted_glm(th, st, ob, w, G=600, ctx=ctx, outputs=ALL, probs=(0.5,), truth=th[1])
    for k in gold:
        assert same(gold[k], gnew[k]), k


def batch_of(K, nA, P, G=16):
    """gl_batch of csrc/glm.hip for a *_summary call: the targets of one workspace batch of 256 MiB"""
    D = nA + P
    nch = min((K + 255) // 256, 64)
    CH = (K + nch - 1) // nch
    nch = (K + CH - 1) // CH
    rec = 3 * 32 * 32 + 4 * 32 + 4
    nchunk = (G + 511) // 512
    per = K * D * 8 + K * 8 + nch * (D + 3) * 8 + nch * D * D * 8 + rec * 8 + K * P * 8 + 3 * K * 8 + P * 32 + P * nchunk * 12 + P * 32
    return (256 << 20) // per


def test_a_call_that_spans_two_workspace_batches(ctx):
    """A batch holds floor(2^28 / bytes of a target) targets.  The bytes grow with K (n + 2 P + 4) 8, so the largest P and number of
    components, 32 and 32, need the smallest K: K = 1393 is the first at which 200 targets do not fit (K = 1392: 200 fit exactly),
    and the test takes K = 1400, where a target takes 1 347 888 bytes and a batch holds 199.  B = 200 is cut after target 198."""
    assert batch_of(1392, 32, 32) == 200 and batch_of(1393, 32, 32) == 199 and batch_of(1400, 32, 32) == 199
    X, Y = GC.table(2400, 32, 32, 33)
    B, K = 200, 1400
    T = X[np.arange(B) * 11] + 0.05
    truth = Y[np.arange(B) * 11]
    F = TG.fit(ctx, X, Y, 32)
    import torch
    model = F["model"].clone()
    model[0] = 32.0                                          # (the batch is sized by A, whatever the fit's own ncomp)
    r = run_dev(ctx, F, T, K, None, (0.025, 0.5, 0.975), truth, outputs=("status", "mean"), model=model)
    assert np.array_equal(r["status"], np.zeros(B)) and np.all(np.isfinite(r["quant"])) and np.all(np.isfinite(r["cdf"]))
    for b in (198, 199):
        alone = run_dev(ctx, F, T[b:b + 1], K, None, (0.025, 0.5, 0.975), truth[b:b + 1], outputs=("status", "mean"), model=model)
        for k in ("quant", "cdf", "mean"):
            assert same(alone[k][0], r[k][b]), (k, b)


def test_status_bits(ctx):
    """a duplicated parameter column (bit 0), K = P + 1 (bit 1) and a NaN parameter (bit 2): all-NaN quant and cdf for that target,
    the other targets of the batch as they were"""
    from abcsmc_amd import device
    X, Y = GC.table(800, 5, 3, 21)
    T = X[[3, 30]] + 0.05
    truth = Y[[3, 30]]
    F = TG.fit(ctx, X, Y, 2)
    pr = (0.1, 0.5)
    good = run_dev(ctx, F, T, 40, None, pr, truth)
    assert np.array_equal(good["status"], [0, 0]) and np.all(np.isfinite(good["quant"])) and np.all(np.isfinite(good["cdf"]))
    Yd = Y.copy()
    Yd[:, 2] = Yd[:, 0]
    r = run_dev(ctx, dict(F, Yd=device.colmajor(Yd, DEV)), T, 40, None, pr, truth)
    assert np.array_equal(r["status"], [1, 1]) and np.all(np.isnan(r["quant"])) and np.all(np.isnan(r["cdf"]))
    r = run_dev(ctx, F, T, 4, None, pr, truth)
    assert np.array_equal(r["status"], [2, 2]) and np.all(np.isnan(r["quant"])) and np.all(np.isnan(r["cdf"]))
    Yn = Y.copy()
    row = int(good["idx"][0, 7])
    assert row not in good["idx"][1]
    Yn[row, 1] = np.nan
    r = run_dev(ctx, dict(F, Yd=device.colmajor(Yn, DEV)), T, 40, None, pr, truth)
    assert np.array_equal(r["status"], [4, 0]) and np.all(np.isnan(r["quant"][0])) and np.all(np.isnan(r["cdf"][0]))
    for k in ALL + ("quant", "cdf"):
        assert same(r[k][1], good[k][1]), k


def test_refused_arguments(ctx):
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -4
    X, Y = table(seed=22)
    F = TG.fit(ctx, X, Y, 2)
    from abcsmc_amd import device
    T = device.colmajor(X[:2], DEV)
    nan = float("nan")
    out = torch.full((4096,), -7.0, dtype=torch.float64, device=DEV)     # every output of every refused call
    idx = torch.full((2 * 20,), -7, dtype=torch.int64, device=DEV)
    th = torch.zeros(40 * 33, dtype=torch.float64, device=DEV)
    keep = []

    def summ(probs=(0.5,), nq=None, quant=True, cdf=False, truth=False):
        pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64))
        keep.append(pr)
        return _lib.Summary(pr.ctypes.data if pr.size else None, pr.size if nq is None else nq, out.data_ptr() if truth else None,
                            out.data_ptr() + 8 * 512 if quant else None, out.data_ptr() + 8 * 2048 if cdf else None)

    def desc(G=16, mean=False):
        d = _lib.Glm(G, 3.0, 1.0, None, *([None] * len(ALL)))
        if mean:
            d.mean = out.data_ptr() + 8 * 3072
        return d

    def dev(d, sm, name="abc_glm_rank_targets_summary_dev"):
        rc = L.abc_glm_rank_targets_summary_dev(C.byref(d), C.byref(sm) if sm is not None else None, ctx.handle, F["Xd"].data_ptr(), 400,
                                                F["Yd"].data_ptr(), 400, 400, 6, 3, F["model"].data_ptr(), 2, T.data_ptr(), 2, 2, None, 20,
                                                idx.data_ptr(), None)
        return rc, name

    def gen(d, sm, name="abc_glm_weighted_summary_dev"):
        rc = L.abc_glm_weighted_summary_dev(C.byref(d), C.byref(sm) if sm is not None else None, ctx.handle, th.data_ptr(), 40,
                                            th.data_ptr(), 40, 40, 3, 2, th.data_ptr(), None)
        return rc, name

    def refused(call, d, sm, code):
        rc, name = call(d, sm)
        msg = L.abc_last_error(ctx.handle)
        msg = msg.decode() if isinstance(msg, bytes) else msg
        assert rc == code and msg and msg.startswith(name + ":"), (rc, code, msg)

    for call in (dev, gen):
        refused(call, desc(), None, INVALID)                                   # NULL sum
        refused(call, desc(), summ(quant=False), INVALID)                      # nothing asked for
        refused(call, desc(), summ(probs=(), nq=0), INVALID)
        refused(call, desc(), summ(probs=np.full(65, 0.5)), INVALID)
        for bad in (0.0, 1.0, nan, -0.1):
            refused(call, desc(), summ(probs=(0.5, bad)), INVALID)
        refused(call, desc(), summ(quant=False, cdf=True), INVALID)            # cdf without truth
        refused(call, desc(G=1), summ(), INVALID)                              # G is checked though no grid output is asked for
        with ctx.param_transf(*_lib.transf_arrays(["log", "none", "none"], None, None)):
            refused(call, desc(), summ(), UNSUPPORTED)
        with ctx.adjust_hcorr(True):
            refused(call, desc(), summ(), UNSUPPORTED)
        with ctx.adjust_ridge([0.1]):
            refused(call, desc(), summ(), UNSUPPORTED)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((idx == -7).all())               # no output was written
    assert dev(desc(), summ())[0] == 0 and dev(desc(mean=True), summ(quant=False))[0] == 0
    torch.cuda.synchronize()
    assert bool((out[512:515] != -7.0).all())


# abc_ws_info's "asked" of the four older entries on the worker's inputs, measured on the commit before the *_summary entries
OLD_ASKED = {"dev": 11300137, "host": 11466617, "gen_host": 105076, "gen_dev": 69644}


def test_entries_keep_to_their_reservation_fresh_and_poisoned(tmp_path):
    """tests/_glm_summary_worker.py as the environment is and under ABC_WS_POISON=ff: the four *_summary entries on a fresh context
    and on one whose arena a larger call has grown; abc_ws_info's peak never exceeds what the entry asked for and reserved, every
    output has the same bytes in all four runs, and the four older entries ask for what they asked for before"""
    runs = {}
    for child in ("plain", "poison"):
        out = str(tmp_path / (child + ".npz"))
        env = dict(os.environ)
        env.pop("ABC_WS_POISON", None)
        if child == "poison":
            env["ABC_WS_POISON"] = "ff"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_glm_summary_worker.py"), out], capture_output=True, text=True,
                           timeout=120, env=env, cwd=ROOT)
        assert p.returncode == 0, (child, p.stdout[-2000:], p.stderr[-3000:])
        with np.load(out) as z:
            runs[child] = {k: z[k] for k in z.files}
    ref = runs["plain"]
    keys = sorted(ref)
    assert len([k for k in keys if k.endswith("|info")]) == 12 and sorted(runs["poison"]) == keys
    for child in runs:
        for k in keys:
            mode, name, field = k.split("|")
            v = runs[child][k]
            if field == "info":
                reserved, asked, peak = (int(x) for x in v)
                print(child, mode, name, "reserved %d asked %d peak %d" % (reserved, asked, peak))
                assert peak <= asked <= reserved, (child, k, v)
                if mode == "old":
                    assert asked == OLD_ASKED[name], (name, asked, OLD_ASKED[name])
            else:
                a = ref["fresh|%s|%s" % (name, field)] if mode != "old" else ref[k]
                assert a.dtype == v.dtype and a.shape == v.shape and a.tobytes() == v.tobytes(), (child, k)


def device_model_posterior(X, Y, T, training_fraction, K, outputs=(), probs=None, truth=None, **kw):
    """the NumPy stand-in for the summaries alone: the model (peaks, c, T) from the older device entry, so that the model's
    rounding does not enter, and quant / cdf from tests/_glm_summary_ref.py"""
    from abcsmc_amd import glm
    r = glm.particle_ranking_PLS_targets_glm(X, Y, T, training_fraction, K, outputs=tuple(outputs) + ("peaks", "c", "T"), **kw)
    B, P = T.shape[0], Y.shape[1]
    r["quant"] = None if probs is None else np.full((B, len(probs), P), np.nan)
    r["cdf"] = None if truth is None else np.full((B, P), np.nan)
    for b in range(B):
        if r["status"][b] == 0:
            s = S.summary(r["peaks"][b], r["c"][b], r["T"][b], probs, None if truth is None else truth[b])
            for k in s:
                r[k][b] = s[k]
    return r


def test_cross_validation_coverage_against_the_numpy_stand_in(ctx, oracle):
    """cross_validate_pls_glm(X, Y, 60, K, seed, coverage=True) on the synthetic table against the same call through a NumPy
    stand-in.  The stand-in takes the model (peaks, c, T) from the older device entry and computes the CDF with F_ref, as the
    accuracy tests do, so that the model's rounding does not enter; truth_cdf is then held to (K + 8) 2^-52 = 2.4e-14 (measured:
    1.1e-16).  The stand-in that also fits and ranks in NumPy (the oracle's fit, tests/_glm_ref.py) is held to the same bar: the
    rounding of the two fits moves truth_cdf by 4.4e-15 on this table.
    Ties.  A target counts in ci95 when 0.025 <= u <= 0.975, both ends included; with truth_cdf equal to the bar, ci95 is equal
    unless a value of the stand-in lies within the bar of an end (such parameters are left out of the comparison, and none does
    here); coverage_ks sorts the finite values and is a maximum of differences of them, so it is equal to the bar as well."""
    from abcsmc_amd import glm, synthetic
    X, Y = synthetic.Workload(8, 4).rows(0, 2000)
    K, n = 100, 60
    bar = (K + 8) * 2.0 ** -52
    cv = glm.cross_validate_pls_glm(X, Y, n, K, 7, coverage=True, ctx=ctx)
    ref = glm.cross_validate_pls_glm(X, Y, n, K, 7, coverage=True, ctx=ctx, posterior=device_model_posterior)
    far = glm.cross_validate_pls_glm(X, Y, n, K, 7, coverage=True, posterior=S.numpy_posterior(oracle, R, GC))
    assert np.all(cv["status"] == 0) and np.all(ref["status"] == 0) and cv["truth_cdf"].shape == (n, 4)
    assert np.array_equal(cv["idx"], ref["idx"]) and same(cv["post_mean"], ref["post_mean"]) and same(cv["pred_error"], ref["pred_error"])
    d = np.abs(cv["truth_cdf"] - ref["truth_cdf"]).max()
    print("truth_cdf: device against the stand-in %.3e (bar %.3e); against the all-NumPy stand-in %.3e, ci95 %s %s, coverage_ks %s %s"
          % (d, bar, np.abs(cv["truth_cdf"] - far["truth_cdf"]).max(), cv["ci95"], far["ci95"], cv["coverage_ks"], far["coverage_ks"]))
    assert d <= bar
    edge = np.minimum(np.abs(ref["truth_cdf"] - 0.025), np.abs(ref["truth_cdf"] - 0.975)).min(axis=0) <= bar
    assert not edge.any()
    assert np.array_equal(cv["ci95"], ref["ci95"])
    assert np.abs(cv["coverage_ks"] - ref["coverage_ks"]).max() <= bar
    assert np.array_equal(far["idx"], cv["idx"].astype(np.int64)) and np.abs(cv["truth_cdf"] - far["truth_cdf"]).max() <= bar
    assert np.array_equal(cv["ci95"], far["ci95"]) and np.abs(cv["coverage_ks"] - far["coverage_ks"]).max() <= bar
