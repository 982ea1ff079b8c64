"""Every branch of the batched-targets selection (abcsmc_amd/csrc/targets.hip, launch_rank_targets) against a reference that is
independent of the device, bit for bit, on FABRICATED model records (test_gpu_project._fabricate: chosen M, A and header, zero-variance
metrics, loadings over many decades, NaN wherever the ranking does not read): no fit is on the path.

Per call (_run): abc_rank_targets_dev directly; X with a leading dimension beyond N and NaN gap rows, the targets with ldt > B and NaN
gap columns, idx and dist inside sentinel-filled buffers with guard words on both sides, the model record compared afterwards.  The case
states what it means to reach -- the candidate kernel's width and rows per thread, the plan, the kernel that scores the rows, the
chunks, the target groups -- and _run holds that to the mirror (tests/_targets_model.py) before the call.  EVERY target is checked: idx
must equal the first K of the reference order (stable by (distance, row), the excluded row removed), dist its distances as uint64
views, and ctx.targets_fallbacks() must rise by exactly the number of targets for which the exact host model of the selection says
the device gives up.  Every call is made twice on one context: the candidate order depends on atomics, the result must not.

Reference distances: the oracle's projection with observed scores from exact fma chains (B <= 16), or, with one metric and one
component, plain numpy (_targets_model.m1_distances), which is exact there and makes thousands of targets cheap.  Nothing here
compares with a tolerance.  test_cases_cover_every_branch holds the union of what the cases state to the list of branches."""
import numpy as np
import pytest

import _pls_ref as PR
import _targets_model as TM
from test_gpu_project import _fabricate
from test_gpu_stats import _dev_cols

pytestmark = pytest.mark.gpu

GUARD = 8
IDX_SENTINEL = 0x5A5A5A5A5A5A5A5A
DIST_SENTINEL = -1.0            # (no distance is negative; NaN is a value the rows of test_keys produce)
P = 3
STATED = []                     # what the cases state (filled while the module is collected): the coverage test reads it

# A -> (kc, rows per thread, the kernel that scores 1000 aligned rows of even leading dimension): the widths' table, restated
WIDTHS = {1: (1, 4, TM.ROW_SCORES), 2: (2, 4, TM.ROW_SCORES), 3: (4, 4, TM.ROW_SCORES), 5: (8, 4, ("dist2_lds", 8)),
          9: (16, 2, ("dist2_lds", 16)), 17: (32, 1, ("mfma", 2, "stage")), 33: (0, 1, TM.ROW_SCORES), 40: (0, 1, TM.ROW_SCORES)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _state(**want):
    STATED.append(want)
    return want


def _record(n, M, A, header, seed, **kw):
    rec = _fabricate(n, M, P, A, header, seed, **kw)
    rec.update(M=M, A=A, nc=TM.tg_ncomp(header, A))
    return rec


def _oracle_ref(oracle, rec, X, T):
    """b -> the N reference distances of target b: exact observed scores, the oracle's projection"""
    cache = {}

    def ref(b):
        if b not in cache:
            if rec["nc"] == 0:
                cache[b] = np.zeros(X.shape[0])
            else:
                o = TM.target_scores(T[b], rec["mean"], rec["sd"], rec["R"], rec["nc"])
                cache[b] = oracle.project_distance(X, rec["mean"], rec["sd"], rec["R"], rec["nc"], o)
        return cache[b]
    return ref


def _m1(N, z, tz, seed):
    """a one-metric, one-component record, rows with z-scores (about) z and targets (about) tz -> rec, X, T, reference"""
    rec = _record(N, 1, 1, 1, seed)
    mean, sd, r = rec["mean"][0], rec["sd"][0], rec["R"][0, 0]
    assert sd != 0 and r != 0
    X = np.asfortranarray(TM.m1_x(z, mean, sd).reshape(N, 1))
    T = np.ascontiguousarray(TM.m1_x(np.asarray(tz, dtype=np.float64), mean, sd).reshape(-1, 1))
    return rec, X, T, lambda b: TM.m1_distances(X[:, 0], mean, sd, r, T[b, 0])


def _expect(rec, X, T, K, ref, want, ex, ldx, aligned, verdicts):
    """the CPU half of _run: holds what the case states to the mirror and the model -> (the model's verdicts, per target the
    reference's first K rows and their distances)"""
    N, M = X.shape
    B, A = T.shape[0], rec["A"]
    any_excl = ex is not None and bool((ex >= 0).any())
    plan = TM.launch_plan(N, M, A, B, K, any_excl, ldx, aligned)
    plan["groups"] = "one" if plan["groups"] == [1] else "several" if min(plan["groups"]) > 1 else "both"
    got = {k: plan[k] for k in want if k in plan}
    assert got == {k: want[k] for k in got}, "the case does not reach what it means to: %s" % (plan,)
    ver, orders, drop = [], [], set()
    for b in range(B):
        d = ref(b)
        e = int(ex[b]) if (ex is not None and ex[b] >= 0) else None
        ver.append(TM.select_model(d, K, e, any_excl)[0])
        o = TM.reference_order(d, e)[:K]
        orders.append((o, d[o]))
        if e is not None and ver[b] != "ok":             # k_tg_drop: the excluded row among the K + 1 selected, or not
            drop.add("inside" if e in TM.reference_order(d)[:K + 1] else "outside")
    if verdicts is not None:
        assert ver == list(verdicts), "the inputs do not land where they are meant to: %s" % (
            ver if B <= 16 else [(b, ver[b]) for b in range(B) if ver[b] != verdicts[b]][:20],)
    assert "verdicts" not in want or set(ver) == want["verdicts"], (set(ver), want["verdicts"])
    assert "drop" not in want or drop == want["drop"], (drop, want["drop"])
    return ver, orders


def _run(gpu_ctx, rec, X, T, K, ref, want, excl=None, ldx=None, xoff=0, verdicts=None, classes=False):
    """abc_rank_targets_dev, twice, checked as the module's docstring says -> (idx (B, K), dist (B, K), the model's verdicts).
    want: what the call must reach by the mirror (and, under "verdicts" and "drop", the sets of the model's verdicts and of
    k_tg_drop's two cases it must produce); verdicts: the per-target verdicts the case means to produce (None: whatever the
    model says); classes: behind a target's finite prefix only the classes (+inf, then NaN) are compared, rows ascending inside a
    run of equal device keys."""
    N, M = X.shape
    B, A = T.shape[0], rec["A"]
    ldx = N + 2 + (N & 1) if ldx is None else ldx
    ldt = B + 3
    ex = None if excl is None else np.asarray(excl, dtype=np.int64)
    ver, orders = _expect(rec, X, T, K, ref, want, ex, ldx, xoff % 2 == 0, verdicts)
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    assert PR.model_layout(M, P, A)["len"] == L.abc_model_len(M, P, A) == rec["model"].size
    tX, pX = _dev_cols(X, ldx, xoff)
    tT, pT = _dev_cols(T, ldt, 0)
    assert tX.data_ptr() % 16 == 0
    nfail = sum(v != "ok" for v in ver)
    model = torch.from_numpy(rec["model"]).to("cuda:0")
    exd = torch.from_numpy(ex).to("cuda:0") if ex is not None else None
    outs = []
    for rep in range(2):
        ibuf = torch.full((2 * GUARD + B * K,), IDX_SENTINEL, dtype=torch.int64, device="cuda:0")
        dbuf = torch.full((2 * GUARD + B * K,), DIST_SENTINEL, dtype=torch.float64, device="cuda:0")
        gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        before = gpu_ctx.targets_fallbacks()
        gpu_ctx.check(L.abc_rank_targets_dev(gpu_ctx.handle, pX, ldx, None, N, N, M, P, model.data_ptr(), A, pT, ldt, B,
                                             exd.data_ptr() if exd is not None else None, K, ibuf.data_ptr() + 8 * GUARD,
                                             dbuf.data_ptr() + 8 * GUARD, None))
        torch.cuda.synchronize()
        fell = gpu_ctx.targets_fallbacks() - before
        print("N=%d M=%d A=%d B=%d K=%d: fallbacks %d, model %d" % (N, M, A, B, K, fell, nfail))
        assert fell == nfail, "%d targets took the exact path, the model says %d (%s)" % (
            fell, nfail, ver if B <= 16 else [(b, ver[b]) for b in range(B) if ver[b] != "ok"][:20])
        i, d = ibuf.cpu().numpy(), dbuf.cpu().numpy()
        for g in (slice(0, GUARD), slice(GUARD + B * K, None)):
            assert (i[g] == IDX_SENTINEL).all() and (d[g] == DIST_SENTINEL).all(), "written outside idx / dist"
        outs.append((i[GUARD:GUARD + B * K].reshape(B, K).copy(), d[GUARD:GUARD + B * K].reshape(B, K).copy()))
    assert np.array_equal(_bits(model.cpu().numpy()), _bits(rec["model"])), "the model record was written to"
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1])), "two calls differ"
    idx, dist = outs[0]
    for b in range(B):
        o, dd = orders[b]
        n = int(np.isfinite(dd).sum()) if classes else K
        bad = np.flatnonzero(idx[b, :n] != o[:n])
        assert bad.size == 0, "target %d (%s): %d of %d ranks differ, first at %d: row %d, reference %d" % (
            b, ver[b], bad.size, n, bad[0], idx[b, bad[0]], o[bad[0]])
        assert np.array_equal(_bits(dist[b, :n]), _bits(dd[:n])), "target %d (%s): distances differ in bits" % (b, ver[b])
        if n < K:
            t, ti = dist[b, n:], idx[b, n:]
            assert np.array_equal(np.isposinf(t), np.isposinf(dd[n:])) and np.array_equal(np.isnan(t), np.isnan(dd[n:])), (b, t, dd[n:])
            same = _bits(t)[1:] == _bits(t)[:-1]
            assert (ti[1:][same] > ti[:-1][same]).all() and (ti >= 0).all() and (ti < X.shape[0]).all()
            assert np.array_equal(np.sort(ti[np.isposinf(t)]), np.sort(o[n:][np.isposinf(dd[n:])]))
    return idx, dist, ver


def _targets(rec, X, B, seed):
    """B targets: rows of X (distance exactly 0), a duplicate of an earlier target, one 1e4 sd outside the cloud, points of the cloud"""
    rng = np.random.default_rng(seed)
    N, M = X.shape
    T = rec["mean"] + rec["sdn"] * rng.normal(size=(B, M))
    T[0] = X[N // 3]
    if B > 2:
        T[2] = T[1]
    if B > 3:
        T[3] = rec["mean"] - 1e4 * rec["sdn"]
    if B > 4:
        T[4] = X[N - 1]
    return np.ascontiguousarray(T)


# ---- widths ------------------------------------------------------------------------------------------------------------------------------
WIDTH_CASES = [(N, A, h) for N in (1000, 4097) for A in WIDTHS for h in ((A, A - 1) if A > 1 else (A,))]
for _N, _A, _h in WIDTH_CASES:
    _state(kc=WIDTHS[_A][0], rpt=WIDTHS[_A][1], plan="exact" if _N == 1000 else "sampled",
           scoring=WIDTHS[_A][2] if _N == 1000 else TM.ROW_SCORES, nchunks=1, groups="several", ragged=False)


@pytest.mark.parametrize("N,A,header", WIDTH_CASES, ids=lambda v: str(v))
def test_widths(gpu_ctx, oracle, N, A, header):
    """every instance of k_tg_cand on both plans; N = 4097 is odd, so its rows are scored by k_tg_row_scores"""
    M, B = max(A, 6), 7
    rec = _record(N, M, A, header, seed=31 * N + 7 * A + header)
    X = rec["X"]
    T = _targets(rec, X, B, seed=N + A)
    ref = _oracle_ref(oracle, rec, X, T)
    kc, rpt, scoring = WIDTHS[A]
    want = dict(kc=kc, rpt=rpt, plan="exact" if N == 1000 else "sampled", scoring=scoring if N == 1000 else TM.ROW_SCORES,
                nchunks=1, groups="several", ragged=False)
    assert ref(0)[N // 3] == 0.0 and ref(4)[N - 1] == 0.0 and np.array_equal(ref(1), ref(2))
    for K in (1, 17, N // 10, N - 1, N):
        _run(gpu_ctx, rec, X, T, K, ref, want)


# ---- the component-count header -----------------------------------------------------------------------------------------------------------
HEADER_CASES = [(N, h) for N in (1000, 1024, 1025) for h in (0.0, -3.0, 13.0, 2.9)]
for _N, _h in HEADER_CASES:
    _state(kc=8, rpt=4, plan="exact", scoring=("dist2_lds", 8) if _N % 2 == 0 else TM.ROW_SCORES, nchunks=1, groups="several",
           ragged=False, header=_h, verdicts={"ok"} if (_N <= 1024 or _h > 0) else {"bin"})


@pytest.mark.parametrize("N,header", HEADER_CASES, ids=lambda v: str(v))
def test_component_count_header(gpu_ctx, oracle, N, header):
    """model[0] of 0, below 0, beyond A and fractional: tg_ncomp's clamp and truncation (0, 0, A, 2).  Without a component every
    distance is +0: one bin of N keys, selected on the device up to TG_CAP keys and by the exact path beyond"""
    A, M, B = 8, 8, 7
    rec = _record(N, M, A, header, seed=5 * N + int(header * 10) % 97)
    assert rec["nc"] == {0.0: 0, -3.0: 0, 13.0: 8, 2.9: 2}[header]
    X = rec["X"]
    T = _targets(rec, X, B, seed=N)
    ref = _oracle_ref(oracle, rec, X, T)
    want = dict(kc=8, rpt=4, plan="exact", scoring=("dist2_lds", 8) if N % 2 == 0 else TM.ROW_SCORES, nchunks=1, groups="several",
                ragged=False)
    for K in (1, 17, N):
        verdicts = None if rec["nc"] else ["ok" if N <= 1024 else "bin"] * B
        idx, dist, _ = _run(gpu_ctx, rec, X, T, K, ref, want, verdicts=verdicts)
        if rec["nc"] == 0:
            assert not _bits(dist).any() and np.array_equal(idx, np.tile(np.arange(K), (B, 1)))


# ---- the kernel that scores the rows ----------------------------------------------------------------------------------------------------
for _A, _k in ((8, ("dist2_lds", 8)), (16, ("dist2_lds", 16)), (24, ("mfma", 2, "stage"))):
    _state(kc=TM.tg_kc(_A), plan="sampled", scoring=_k, nchunks=1)
    _state(kc=TM.tg_kc(_A), plan="sampled", scoring=TM.ROW_SCORES, nchunks=1)


@pytest.mark.parametrize("A,fused", [(8, ("dist2_lds", 8)), (16, ("dist2_lds", 16)), (24, ("mfma", 2, "stage"))])
def test_scoring_kernels_agree(gpu_ctx, oracle, A, fused):
    """4098 aligned rows of even leading dimension take the projection's fused pass; the same rows 8 bytes off, with an odd leading
    dimension, and without the last one (N = 4097) take k_tg_row_scores: four identical results (the last row lies far outside,
    so that it is in no target's first K)"""
    N, M, B, K = 4098, 24, 5, 300
    rec = _record(N, M, A, A, seed=900 + A)
    X = rec["X"].copy(order="F")
    X[N - 1] = rec["mean"] + 1e3 * rec["sdn"]
    T = _targets(rec, X, 4, seed=A)
    T = np.ascontiguousarray(np.vstack([T, rec["mean"] + 0.5 * rec["sdn"]]))
    ref = _oracle_ref(oracle, rec, X, T)
    base = dict(kc=TM.tg_kc(A), plan="sampled", nchunks=1)
    a = _run(gpu_ctx, rec, X, T, K, ref, dict(base, scoring=fused), ldx=N + 2)
    outs = [_run(gpu_ctx, rec, X, T, K, ref, dict(base, scoring=TM.ROW_SCORES), ldx=N + 2, xoff=1),
            _run(gpu_ctx, rec, X, T, K, ref, dict(base, scoring=TM.ROW_SCORES), ldx=N + 3)]
    Xs = np.asfortranarray(X[:N - 1])
    outs.append(_run(gpu_ctx, rec, Xs, T, K, _oracle_ref(oracle, rec, Xs, T), dict(base, scoring=TM.ROW_SCORES), ldx=N + 2))
    for o in outs:
        assert np.array_equal(o[0], a[0]) and np.array_equal(_bits(o[1]), _bits(a[1]))
    assert (a[0] != N - 1).all()


# ---- the sample's positions -----------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(N, down) for N in (4097, 8191, 8192, 12289) for down in (False, True)]
for _N, _d in SAMPLE_CASES:
    _state(kc=1, rpt=4, plan="sampled", scoring=TM.ROW_SCORES, nchunks=1, groups="several", ragged=False)


@pytest.mark.parametrize("N,down", SAMPLE_CASES, ids=lambda v: str(v))
def test_sample_positions(gpu_ctx, N, down):
    """rows sorted by their distance to target 0, ascending and descending, at strides 1, 2 and 3: the sampled ranks, and with them
    the threshold and the candidate count the model predicts, follow tg_sample_row exactly"""
    rng = np.random.default_rng(N)
    z = np.sort(np.abs(rng.normal(size=N)))
    z = z[::-1].copy() if down else z
    rec, X, T, ref = _m1(N, z, [0.0, 0.7, -2.0, 0.7], seed=N + down)
    d0 = ref(0)
    assert (np.diff(d0) <= 0).all() if down else (np.diff(d0) >= 0).all()
    want = dict(kc=1, rpt=4, plan="sampled", scoring=TM.ROW_SCORES, nchunks=1, groups="several", ragged=False)
    s = TM.select_detail(d0, 50)
    row = TM.tg_sample_row(4095 - s["q"] if down else s["q"], N, 4096)       # the sampled row of rank q among the sample
    assert s["tkey"] == int(TM.key_of(d0[[row]])[0]) and s["c"] == (N - row if down else row + 1)
    _run(gpu_ctx, rec, X, T, 50, ref, want)
    _run(gpu_ctx, rec, X, T, 49, ref, want, excl=[int(np.argmin(d0)), -1, 5, 4000])


@pytest.mark.parametrize("N,shift", [(8192, -1), (8192, 1), (12289, -1), (12289, 1)])
def test_sample_offset(gpu_ctx, N, shift):
    """300 rows right at target 0 sit one row beside sampled rows (before them: shift -1, behind: +1).  The sample does not see
    them, the threshold is that of the ordinary rows, and they pass it with everything else: selected on the device.  A sample taken
    one row off would hold all of them and put the threshold among them: fewer than K candidates (the model, on the rolled rows)"""
    K = 100
    rng = np.random.default_rng(N + shift)
    z = 0.5 + np.abs(rng.normal(size=N))
    s = TM.sample_rows(N, 4096)
    z[s[500:800] + shift] = rng.uniform(0.0, 1e-3, size=300)
    rec, X, T, ref = _m1(N, z, [0.0, 0.0, 2.0], seed=N)
    assert TM.select_model(np.roll(ref(0), -shift), K)[:2] == ("short", TM.tg_plan(N, K, False)[1] + 1)
    want = dict(kc=1, rpt=4, plan="sampled", scoring=TM.ROW_SCORES, nchunks=1, groups="several", ragged=False)
    _run(gpu_ctx, rec, X, T, K, ref, want, verdicts=["ok"] * 3)
    _run(gpu_ctx, rec, X, T, K - 1, ref, want, excl=[int(s[600] + shift), -1, 7], verdicts=["ok"] * 3)


# ---- the give-ups -----------------------------------------------------------------------------------------------------------------------
def _near(ref, b, rank):
    return int(TM.reference_order(ref(b))[rank])


def _less(want, *keys):
    return {k: v for k, v in want.items() if k not in keys}


W_GIVE_UP = {v: _state(kc=1, rpt=4, plan="exact" if v == "bin" else "sampled", scoring=TM.ROW_SCORES, nchunks=1, groups="several",
                       ragged=False, verdicts={v, "ok"}, drop={"inside", "outside"}) for v in ("overflow", "short", "bin")}


@pytest.mark.parametrize("far,K,verdict", [("sample", 100, "overflow"), ("others", 3000, "short")])
def test_give_up_sampled(gpu_ctx, far, K, verdict):
    """N = 8192: the sampled (odd) rows 100 units farther from target 0 than the others -- the threshold lets every even row through,
    4183 candidates for a segment of 579 -- and the other way round -- only sampled rows pass, 1632 for K = 3000.  Targets half way
    between the two halves see them at the same distances, an ordinary sample, and must NOT fall back.  With exclusion: a row
    inside the first K, the (K + 1)-th, the farthest one, and none (-1), on targets that give up (k_tg_drop with and without the row
    among the K + 1 selected) and on targets that do not."""
    N = 8192
    z = TM.split_rows(N, 1 if far == "sample" else 2, far)
    rec, X, T, ref = _m1(N, z, [0.0] * 4 + [51.0, 51.0, 51.002, 50.998], seed=11)
    want = W_GIVE_UP[verdict]
    v = TM.select_model(ref(0), K)
    assert v[:3] == (("overflow", 4183, 579) if far == "sample" else ("short", 1632, 4166))
    verdicts = [verdict] * 4 + ["ok"] * 4
    _run(gpu_ctx, rec, X, T, K, ref, _less(want, "drop"), verdicts=verdicts)
    Kx = K - 1
    ex = [_near(ref, 0, 3), _near(ref, 1, Kx), _near(ref, 2, N - 1), -1, _near(ref, 4, 3), _near(ref, 5, Kx), _near(ref, 6, N - 1), -1]
    _run(gpu_ctx, rec, X, T, Kx, ref, want, excl=ex, verdicts=verdicts)


@pytest.mark.parametrize("K", [1, 1200, 1501, 2999])
def test_give_up_bins(gpu_ctx, K):
    """N = 3000, 1500 identical nearest rows: one bin above TG_CAP at or before the K-th key, whatever K.  Targets on the other side
    of the set have the ties as their 1500 FARTHEST rows: they must not fall back until K reaches the ties"""
    N = 3000
    z = TM.tied_rows(N, 1500, 4)
    rec, X, T, ref = _m1(N, z, [0.0, 0.0, 0.0, 0.25, 9.0, 9.0, 9.5, 8.5], seed=12)
    assert np.count_nonzero(ref(3) == 0.0) == 1500
    want = W_GIVE_UP["bin"]
    verdicts = ["bin"] * 4 + (["ok"] * 4 if K <= 1500 else ["bin"] * 4)
    _run(gpu_ctx, rec, X, T, K, ref, _less(want, "drop") if K <= 1500 else _less(want, "drop", "verdicts"), verdicts=verdicts)
    ex = [_near(ref, 0, 0), _near(ref, 1, K), _near(ref, 2, N - 1), -1, _near(ref, 4, 0), _near(ref, 5, K), _near(ref, 6, N - 1), -1]
    _run(gpu_ctx, rec, X, T, K, ref, want if K <= 1500 else _less(want, "drop", "verdicts"), excl=ex, verdicts=verdicts)


_state(kc=1, rpt=4, plan="exact", verdicts={"ok"}, nchunks=1)
_state(kc=1, rpt=4, plan="sampled", verdicts={"bin", "ok"}, nchunks=1)


def test_ordinary_and_pad_key(gpu_ctx):
    """ordinary rows at N = 3000 never fall back (K = 1, 17, N, and N - 1 with an exclusion); at N = 4097 with K = N - 1 and an excluded
    row inside the sample the threshold is the pad key, the bins span the whole key range and every target falls back"""
    N = 3000
    rec, X, T, ref = _m1(N, TM.ordinary_rows(N, 5), [0.3, -1.0, 2.5], seed=13)
    want = dict(kc=1, rpt=4, plan="exact", scoring=TM.ROW_SCORES, nchunks=1)
    for K in (1, 17, N):
        _run(gpu_ctx, rec, X, T, K, ref, want, verdicts=["ok"] * 3)
    _run(gpu_ctx, rec, X, T, N - 1, ref, want, excl=[_near(ref, 0, 40), -1, _near(ref, 2, N - 1)], verdicts=["ok"] * 3)
    N = 4097
    rec, X, T, ref = _m1(N, TM.ordinary_rows(N, 6), [0.1, -0.5, 1.0], seed=14)
    want = dict(kc=1, rpt=4, plan="sampled", scoring=TM.ROW_SCORES, nchunks=1)
    _run(gpu_ctx, rec, X, T, N - 1, ref, want, excl=[10, 10, 4000], verdicts=["bin"] * 3)
    _run(gpu_ctx, rec, X, T, 50, ref, want, excl=[10, -1, 4096], verdicts=["ok"] * 3)


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------
_state(kc=8, rpt=4, plan="exact", scoring=("dist2_lds", 8), nchunks=1)
_state(kc=8, rpt=4, plan="sampled", scoring=TM.ROW_SCORES, nchunks=1)


@pytest.mark.parametrize("N", [3000, 4097])
def test_keys(gpu_ctx, oracle, N):
    """distances of exactly 0, duplicated targets, a target 1e4 sd outside; rows with a +inf metric (distance +inf: behind every
    finite row) and with a NaN metric (NaN: behind those); and the single-target device call -- abc_project_distance_dev on the
    record with the target's scores as the observed ones, abc_select_smallest_dev -- bit for bit, which is the existing contract"""
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    M = A = 8                                                           # (nothing padded: +inf stays +inf in the single call too)
    B = 6
    rec = _record(N, M, A, A, seed=N)
    X = rec["X"].copy(order="F")
    live = rec["live"]
    inf_rows, nan_rows = [5, 700, N - 2], [6, 64, 1999, N - 1]
    X[inf_rows, live[0]] = np.inf
    X[nan_rows, live[1]] = np.nan
    X[8, rec["zv"][0]] = np.nan                                         # (a zero-variance metric is not read into the score)
    T = _targets(rec, X, B, seed=3 * N)
    T[4] = X[10]                                                        # (row N - 1 holds a NaN: no target)
    ref = _oracle_ref(oracle, rec, X, T)
    d = ref(1)
    assert np.isposinf(d[inf_rows]).all() and np.isnan(d[nan_rows]).all() and np.isfinite(d).sum() == N - 7
    want = dict(kc=8, rpt=4, plan="exact" if N == 3000 else "sampled", scoring=("dist2_lds", 8) if N == 3000 else TM.ROW_SCORES,
                nchunks=1, groups="several", ragged=False)
    for K in (17, N - 7, N - 4, N):
        idx, dist, _ = _run(gpu_ctx, rec, X, T, K, ref, want, classes=True)
        if K != N:
            continue
        # the single-target call, target by target
        tX, pX = _dev_cols(X, N + 2 + (N & 1), 0)
        lay = PR.model_layout(M, P, A)
        for b in range(B):
            m = rec["model"].copy()
            m[lay["oscore"]:lay["oscore"] + A] = TM.target_scores(T[b], rec["mean"], rec["sd"], rec["R"], A)
            md = torch.from_numpy(m).to("cuda:0")
            dd = torch.empty(N, dtype=torch.float64, device="cuda:0")
            si = torch.empty(N, dtype=torch.int64, device="cuda:0")
            sd = torch.empty(N, dtype=torch.float64, device="cuda:0")
            gpu_ctx.check(L.abc_project_distance_dev(gpu_ctx.handle, pX, N, N + 2 + (N & 1), M, P, A, md.data_ptr(), 0, dd.data_ptr()))
            gpu_ctx.check(L.abc_select_smallest_dev(gpu_ctx.handle, dd.data_ptr(), N, N, 0, si.data_ptr(), sd.data_ptr()))
            torch.cuda.synchronize()
            assert np.array_equal(si.cpu().numpy(), idx[b]), "target %d: the single-target call ranks otherwise" % b
            assert np.array_equal(_bits(sd.cpu().numpy()), _bits(dist[b])), "target %d: ... with other distances" % b


# ---- chunks and groups ---------------------------------------------------------------------------------------------------------------
_state(kc=1, rpt=4, plan="exact", scoring=TM.ROW_SCORES, nchunks=2, groups="several", ragged=True, verdicts={"bin", "ok"},
       drop={"inside", "outside"})


def test_two_chunks(gpu_ctx):
    """N = 4095, B = 5100, K = 33: two chunks of 5042 and 58 targets (the `+ c0` offsets of the scores, thresholds, exclusions, counters,
    flags and outputs), 505 target groups of 10 with a last group of 2 in the first chunk, 58 groups of one in the second.  The last
    target of chunk 0 and the first of chunk 1 sit on 1500 tied rows and give up, one with an excluded row among its K + 1 nearest,
    one with a far one; exclusions on both sides of the boundary; every target checked"""
    N, B, K = 4095, 5100, 33
    rng = np.random.default_rng(50)
    z = TM.tied_rows(N, 1500, 51)
    tz = rng.uniform(3.2, 5.0, size=B)
    tz[5041] = tz[5042] = 0.25
    tz[7] = tz[3]                                                       # duplicates, and rows of the set
    tz[5050] = z[0]
    tz[100] = z[2]
    rec, X, T, ref = _m1(N, z, tz, seed=52)
    ex = np.full(B, -1, dtype=np.int64)
    pick = rng.choice(B, size=600, replace=False)
    ex[pick] = rng.integers(0, N, size=600)
    for b in (0, 5039, 5040, 5043, 5099):
        ex[b] = _near(ref, b, b % 7)                                    # inside the first K
    ex[5041] = _near(ref, 5041, 5)                                      # a tied row, among the K + 1 selected
    ex[5042] = _near(ref, 5042, N - 1)                                  # the farthest row
    verdicts = ["ok"] * B
    verdicts[5041] = verdicts[5042] = "bin"
    want = dict(kc=1, rpt=4, plan="exact", C=4095, bc=5042, scoring=TM.ROW_SCORES, nchunks=2, groups="several", ragged=True)
    plan = TM.launch_plan(N, 1, 1, B, K, True, N + 3, True)
    assert [(c["c0"], c["nb"], c["groups"], c["tgs"], c["last"]) for c in plan["chunks"]] == [(0, 5042, 505, 10, 2), (5042, 58, 58, 1, 1)]
    _run(gpu_ctx, rec, X, T, K, ref, want, excl=ex, verdicts=verdicts)


# ---- second trips, one group ----------------------------------------------------------------------------------------------------------
_state(kc=1, rpt=4, plan="sampled", scoring=TM.ROW_SCORES, nchunks=1, groups="one", ragged=False, second_trip=True,
       verdicts={"overflow", "ok"}, drop={"inside"})


def test_second_trips_and_one_group(gpu_ctx):
    """N = 2 097 409 (odd), B = 3, K = 1000: k_tg_row_scores runs and takes a second trip (N > 4096 x 256), 2049 row blocks make one
    target group of the three targets, and target 0 -- the sampled rows within half a unit of it moved away, so its threshold lets
    a third of the rows through -- gives up, so k_tg_dist_one takes its second trip too"""
    N, B, K = 2097409, 3, 1000
    rng = np.random.default_rng(60)
    z = rng.normal(size=N)
    s = TM.sample_rows(N, 4096)
    assert s[0] == 256 and s[1] - s[0] == 512
    t0 = -1.5
    move = s[np.abs(z[s] - t0) < 0.5]
    z[move] = 50.0 + rng.uniform(size=move.size)
    rec, X, T, ref = _m1(N, z, [t0, 1.0, 0.2], seed=61)
    cache = {}
    cref = lambda b: cache[b] if b in cache else cache.setdefault(b, ref(b))
    want = dict(kc=1, rpt=4, plan="sampled", scoring=TM.ROW_SCORES, nchunks=1, groups="one", ragged=False, second_trip=True)
    ex = [int(TM.reference_order(cref(0))[10]), -1, -1]
    _run(gpu_ctx, rec, X, T, K, cref, want, excl=ex, verdicts=["overflow", "ok", "ok"])


# ---- the smallest calls ---------------------------------------------------------------------------------------------------------------
_state(kc=2, rpt=4, plan="exact", scoring=TM.ROW_SCORES, nchunks=1, groups="one", ragged=False)


def test_one_target_and_two_rows(gpu_ctx, oracle):
    """B = 1; K = N = 2 without an exclusion, K = 1 with one, and K = N with one refused"""
    import torch
    from abcsmc_amd import _lib
    L = _lib.lib()
    M, A = 3, 2
    want = dict(kc=2, rpt=4, plan="exact", scoring=TM.ROW_SCORES, nchunks=1, groups="one", ragged=False)
    rec = _record(2, M, A, A, seed=70)
    X = rec["X"]
    T = np.ascontiguousarray(rec["mean"] + rec["sdn"] * np.array([[0.3, -0.2, 0.1]]))
    ref = _oracle_ref(oracle, rec, X, T)
    for K in (1, 2):
        _run(gpu_ctx, rec, X, T, K, ref, want, ldx=5)
    for e in (0, 1):
        idx, _, _ = _run(gpu_ctx, rec, X, T, 1, ref, want, excl=[e], ldx=5)
        assert idx[0, 0] == 1 - e
    tX, pX = _dev_cols(X, 5, 0)
    tT, pT = _dev_cols(T, 4, 0)
    model = torch.from_numpy(rec["model"]).to("cuda:0")
    out = torch.full((2,), IDX_SENTINEL, dtype=torch.int64, device="cuda:0")
    exd = torch.tensor([1], dtype=torch.int64, device="cuda:0")
    before = gpu_ctx.targets_fallbacks()
    rc = L.abc_rank_targets_dev(gpu_ctx.handle, pX, 5, None, 2, 2, M, P, model.data_ptr(), A, pT, 4, 1, exd.data_ptr(), 2,
                                out.data_ptr(), None, None)
    torch.cuda.synchronize()
    msg = L.abc_last_error(gpu_ctx.handle)
    assert rc == -1 and "K = 2 > N - 1 = 1" in (msg.decode() if isinstance(msg, bytes) else str(msg))
    assert (out.cpu().numpy() == IDX_SENTINEL).all() and gpu_ctx.targets_fallbacks() == before
    # one target over several row blocks, and over the rows of one wave
    for N, K in ((1500, 40), (60, 60)):
        rec = _record(N, M, A, A, seed=71 + N)
        T = _targets(rec, rec["X"], 1, seed=N)
        _run(gpu_ctx, rec, rec["X"], T, K, _oracle_ref(oracle, rec, rec["X"], T), want)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_cases_cover_every_branch():
    """the union of what the cases state (each held to the mirror and the model by _run before its call)"""
    S = STATED
    assert {s["kc"] for s in S} == set(TM.KCS) == {1, 2, 4, 8, 16, 32, 0}
    assert {(s["kc"], s["rpt"]) for s in S if "rpt" in s} == {(kc, TM.tg_rpt(kc)) for kc in TM.KCS}
    for plan in ("exact", "sampled"):                                   # every width on both plans
        assert {s["kc"] for s in S if s["plan"] == plan} == set(TM.KCS)
    assert {s["scoring"] for s in S if "scoring" in s} == {TM.ROW_SCORES, ("dist2_lds", 8), ("dist2_lds", 16), ("mfma", 2, "stage")}
    assert {s["nchunks"] for s in S} == {1, 2}
    assert {s["groups"] for s in S if "groups" in s} == {"one", "several"}
    assert any(s.get("ragged") for s in S) and any(s.get("second_trip") for s in S)
    assert set().union(*(s.get("verdicts", set()) for s in S)) == {"ok", "overflow", "short", "bin"}
    assert set().union(*(s.get("drop", set()) for s in S)) == {"inside", "outside"}
    assert {s["header"] for s in S if "header" in s} == {0.0, -3.0, 13.0, 2.9}
