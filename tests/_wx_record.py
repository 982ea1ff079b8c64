"""The per-test record of a Wilcoxon reduction (abc_wx_last_record) against the exact references, for the GPU tests:
run the reduction alone through the staged entry points, compute the references on the device's own model (oracle/abc_oracle.cpp:
orc_pls_wilcoxon_tests -- the residuals are then the same bits on both sides), compare every test of the plan.

What check_record asserts, per test:
  * the plan (response, candidate, optimum) is the reference's;
  * nz equals the reference's count of non-zero differences wherever a level or the sorted path has seen the test;
  * wherever the sum was taken, 2 W is an integer and equals the reference's 2 W;
  * every level's [lo2, hi2] contains the reference's 2 W, and IS the point 2 W for a test whose non-zero differences all have one
    sign (|2 W| = m (m + 1): every bin of any binning then holds keys of one sign -- the one case in which the interval is known
    without knowing the bins, and the one that tells a bound that is too LOOSE, such as p (p - 1) for p (p + 1) in the lower end).  Level 0 has 192 cells, the fine levels 1024 .. 16384 bins; a second fine
    level has more bins than the first.  The intervals of successive levels are NOT asserted to be nested: a level-0 cell whose
    share of the fine bins rounds to none (wx_wave_table: span 0) shares the first bin of the next cell, so the fine bins are not
    a refinement of the cells in that corner and only containment holds for certain (the number of nested pairs is returned);
  * a verdict settled by the bounds (0 / 1) equals the reference verdict from (m, 2 W) through the float64 copy of the decision
    (tests/_wilcoxon_ref.py).  A test whose reference p lies within 1e-9 of 0.1 is left out of this one comparison (the compiler
    may contract the polynomial); the number left out is returned and the callers assert it to be zero for their seeds.
"""
import numpy as np

import _wilcoxon_ref as WR

P_MARGIN = 1e-9


def model_offsets(M, P, A, L):
    off_mean, off_sd = 4, 4 + M + P
    off_R = off_sd + (M + P) + M + A
    off_Q = off_R + M * A
    return dict(mean=off_mean, sd=off_sd, R=off_R, Q=off_Q, per=L - P)


def run_reduction(gpu_ctx, X, Y, obs, A, f=0.5, record=True, both=False):
    """statistics -> model under argmin PRESS -> abc_pls_wilcoxon_dev.  -> dict(m0, m1, path, rec, ntrain[, m1_off]): the model
    record before and after, the per-test record (record=True); both: the same call once more with the record switched off, on the
    same fitted model (m1_off: to be byte-identical with m1) -- behind the recorded call, or in front of it (both="off first")."""
    import torch
    from abcsmc_amd import _lib, device, sharded
    lib = _lib.lib()
    N, M = X.shape
    P = Y.shape[1]
    dev = "cuda:0"
    be = sharded.HipBackend(dev, gpu_ctx)
    dX, dY, dobs = device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev)
    ntrain = int(round(N * f))
    stats = be.zeros(be.stats_len(M, P))
    L = be.model_len(M, P, A)
    model = be.zeros(L + 8)
    be.stats_shift(dX, dY, stats)
    be.stats_accumulate(dX, dY, 0, ntrain, stats)
    be.pls_model(stats, dobs, M, P, A, _lib.RULE_MIN_PRESS, model)
    torch.cuda.synchronize()
    keep = model.clone()
    out = dict(m0=model.cpu().numpy().copy(), ntrain=ntrain, L=L)

    def call():
        gpu_ctx.check(lib.abc_pls_wilcoxon_dev(gpu_ctx.handle, dX.data_ptr(), dY.data_ptr(), N, N, N, M, P, A, ntrain, model.data_ptr()))
        torch.cuda.synchronize()
        return model.cpu().numpy().copy()
    def recorded():
        gpu_ctx.set_wx_record(record)
        try:
            out["m1"] = call()
            out["path"], out["rec"] = gpu_ctx.wx_last_record() if record else (_lib.WX_PATH_NONE, [])
        finally:
            gpu_ctx.set_wx_record(False)

    def plain():
        out["m1_off"] = call()
        assert gpu_ctx.wx_last_record() == (_lib.WX_PATH_NONE, [])
    if not both:
        recorded()
    else:                                # (both == "off first": the plain call before the recorded one)
        for i, step in enumerate((plain, recorded) if both == "off first" else (recorded, plain)):
            if i:
                model.copy_(keep)
                torch.cuda.synchronize()
            step()
    return out


def oracle_inputs(X, Y, m0, A, ntrain):
    """-> (Zx, Zy, R, Q, optima): the validation rows standardised with the device's means and deviations, its loadings and its
    PRESS optima, as the fit left them in the model record m0 -- what the oracle's reduction takes"""
    N, M = X.shape
    P = Y.shape[1]
    L = len(m0) - 8
    o = model_offsets(M, P, A, L)
    mean, sd = m0[o["mean"]:o["mean"] + M + P], m0[o["sd"]:o["sd"] + M + P]
    R = np.asfortranarray(m0[o["R"]:o["R"] + M * A].reshape(A, M).T)
    Q = np.asfortranarray(m0[o["Q"]:o["Q"] + P * A].reshape(A, P).T)
    with np.errstate(divide="ignore", invalid="ignore"):
        Zx = np.where(sd[:M] == 0, 0.0, (X[ntrain:] - mean[:M]) / sd[:M])
        Zy = np.where(sd[M:] == 0, 0.0, (Y[ntrain:] - mean[M:]) / sd[M:])
    return Zx, Zy, R, Q, m0[o["per"]:L].astype(int)


def reference(oracle, X, Y, m0, A, ntrain, want_d=False):
    """the oracle's tests on the device's own model (its loadings, means and deviations as the fit left them in m0)"""
    Zx, Zy, R, Q, optima = oracle_inputs(X, Y, m0, A, ntrain)
    ref = oracle.pls_wilcoxon_tests(Zx, Zy, R, Q, want_d=want_d)
    ref["optima"] = optima
    ref["near"] = [s for s in range(len(ref["p"])) if abs(ref["p"][s] - 0.1) < P_MARGIN]
    return ref


def check_record(path, rec, ref, m1, P, sorted_path=None, plain=True, label=""):
    """-> dict(left_out, nested, pairs, taken, settled, levels): see the module's docstring.  plain: a reduction that looks at every
    test (not the largest-count-first run of a fused generation) -- the counts in the model record m1 then follow from the
    record's verdicts by the rule, and they are the reference's."""
    from abcsmc_amd import _lib
    n = len(ref["seg_j"])
    assert len(rec) == n, (label, len(rec), n)
    if sorted_path is not None:
        assert (path != _lib.WX_PATH_CASCADE) == sorted_path, (label, path)
    left_out = nested = pairs = taken = settled = points = 0
    levels = {}
    for s, r in enumerate(rec):
        where = (label, s, r)
        m, W2 = int(ref["m"][s]), int(ref["W2"][s])
        assert (r["response"], r["candidate"], r["optimum"]) == (int(ref["seg_j"][s]), int(ref["seg_a"][s]), int(ref["astar"][s])), where
        seen = r["n_levels"] > 0 or path != _lib.WX_PATH_CASCADE
        if seen:
            assert r["nz"] == m, (where, m)
        if path == _lib.WX_PATH_SORTED:
            assert r["n_levels"] == 0 and r["verdict"] == 2 and r["w_taken"] == 1, where
        if r["w_taken"]:
            taken += 1
            assert float(2.0 * r["W"]).is_integer() and int(2.0 * r["W"]) == W2, (where, W2)
        assert r["n_levels"] <= _lib.WX_REC_LEVELS, where                  # (more levels than the record keeps: a new path to test)
        prev = None
        for k, (bins, lo2, hi2) in enumerate(r["levels"]):
            levels[bins] = levels.get(bins, 0) + 1
            assert lo2 <= W2 <= hi2, (where, k, W2)
            if m > 0 and abs(W2) == m * (m + 1):                           # every difference of one sign: p = 0 or p = c in every bin of
                points += 1                                                # ANY binning, and the interval is the point 2 W
                assert lo2 == hi2 == W2, (where, k, W2)
            assert bins == 192 or (1024 <= bins <= 16384 and bins & (bins - 1) == 0), where
            if k == 0:
                assert bins == 192, where
            if prev is not None:
                pairs += 1
                nested += int(prev[1] <= lo2 and hi2 <= prev[2])
                if plain and prev[0] != 192 and bins != 192:
                    assert bins > prev[0], where                           # a second fine level: finer bins
            prev = (bins, lo2, hi2)
        assert r["verdict"] in (0, 1, 2, 3), where
        if r["verdict"] in (0, 1):
            assert r["n_levels"] > 0 and r["passed"] == r["verdict"], where
            if s in ref["near"]:
                left_out += 1
            else:
                settled += 1
                assert bool(r["verdict"]) == WR.passes(m, W2), (where, m, W2, ref["p"][s])
        elif r["w_taken"] and s not in ref["near"]:
            assert bool(r["passed"]) == WR.passes(m, W2), (where, m, W2, ref["p"][s])
    if plain:
        L = len(m1) - 8
        per = m1[L - P:L].astype(int).tolist()
        by_record = WR.counts_from_verdicts(ref["seg_j"], ref["seg_a"], [r["passed"] for r in rec], ref["optima"])
        assert per == by_record, (label, per, by_record)
        if not ref["near"]:
            assert per == WR.counts_from_verdicts(ref["seg_j"], ref["seg_a"], ref["p"] > 0.1, ref["optima"]), label
        assert int(m1[0]) == max(per), label
    return dict(left_out=left_out, nested=nested, pairs=pairs, taken=taken, settled=settled, levels=levels, points=points)


def check_few_keys(rec, ref, max_keys=3):
    """Tests with at most max_keys distinct |d| (validation rows copied from a few): there are only 2^(keys - 1) ways for a
    non-decreasing binning to group the keys, so every level's interval must EQUAL the bounds (tests/_wilcoxon_ref.py: bounds2) of
    one of them -- which also tells a bound that is too loose.  ref: with the differences (reference(..., want_d=True)).
    -> the number of intervals that are points although a positive key is among them."""
    import itertools
    points_with_positives = 0
    for s, r in enumerate(rec):
        d = ref["d"][s]
        u = np.unique(np.abs(d[d != 0.0]))
        assert 1 <= u.size <= max_keys, (s, u)
        alts = set()
        for cuts in itertools.product((0, 1), repeat=u.size - 1):           # a cut between two neighbouring keys, or none
            bin_of_unique = np.concatenate([[0], np.cumsum(cuts)]).astype(np.int64)
            call, cpos = WR.bin_counts(d, lambda a: bin_of_unique[np.searchsorted(u, a)], u.size)
            alts.add(WR.bounds2(call, cpos))
        for bins, lo2, hi2 in r["levels"]:
            assert (lo2, hi2) in alts, (s, bins, lo2, hi2, sorted(alts))
            points_with_positives += int(lo2 == hi2 and bool((d > 0.0).any()))
    return points_with_positives


def run_and_check(gpu_ctx, oracle, X, Y, obs, A, f=0.5, label="", both=True):
    """one reduction with the record on (and once more with it off), checked against the oracle.  -> (run, ref, summary)"""
    run = run_reduction(gpu_ctx, X, Y, obs, A, f, record=True, both=both)
    if both:
        assert run["m1"].tobytes() == run["m1_off"].tobytes(), label       # the record changes nothing the reduction leaves
    ref = reference(oracle, X, Y, run["m0"], A, run["ntrain"])
    assert np.array_equal(ref["optima"][ref["seg_j"]], ref["astar"]), label   # (same argmin PRESS on both sides)
    out = check_record(run["path"], run["rec"], ref, run["m1"], Y.shape[1], label=label)
    return run, ref, out
