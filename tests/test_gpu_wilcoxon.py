"""The Wilcoxon reduction (abcsmc_amd/csrc/wilcoxon.hip) test by test against exact references: with the per-test record on
(abc_ctx_set_wx_record / abc_wx_last_record), every (response, candidate) test of the plan is compared with the oracle's
statistic on the device's own model -- the count of non-zero differences and twice the signed rank sum as INTEGERS, every
cascade level's interval of 2 W for containment, every verdict the bounds settled (tests/_wx_record.py says what exactly).
The component counts, which is all the other Wilcoxon tests look at, move only when a statistic sits within a hair of the
threshold; a wrong rank sum or a bound that is too tight by a few ranks moves these comparisons on every data set.

The cases and their data are in tests/_wx_worker.py, the instantiations of the sweep kernel they reach in tests/_wx_dispatch.py.
The switches that force every test through the exact step (ABC_WX_NOBOUNDS) and cap the counter buffer (ABC_WX_BC_CAP_KB) are read
once per process: those runs happen in ONE child process per setting (all its cases; a time limit of its own; no further child is
started after one that ended abnormally), and the tests read what it wrote.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import _wx_dispatch as D
import _wx_record as WXR
import _wx_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF, _RUNS, _CHILD_OUT, _CHILD_FAILED = {}, {}, {}, []

CHILDREN = {      # setting -> (environment, cases, seconds)
    "forced": ({"ABC_WX_NOBOUNDS": "1"}, list(W.CASES_CASCADE) + list(W.CASES_MANY) + list(W.CASES_OUTGROW), 420),
    # (the caps: room for one group of tests of the level in question, not for two -- 1.25 MB + 1 MB against 17 runs x 29 tests x 1024 bins
    # (or 16 tests x 2048 bins) of a fine level at 16 391 rows, 9 MB + 1 MB against 65 runs x 180 tests x 192 cells of level 0 at 65 537; a cap below one group
    # is refused by the library)
    "forced_capped": ({"ABC_WX_NOBOUNDS": "1", "ABC_WX_BC_CAP_KB": "1280"}, list(W.CASES_CASCADE), 300),
    "capped": ({"ABC_WX_BC_CAP_KB": "9216"}, list(W.CASES_MANY), 300),
}
CAP_KB = {"forced": None, "forced_capped": 1280, "capped": 9216, "asis": None}


def _child(setting, tmp_path_factory):
    """the directory the setting's child process wrote its results to (started once)"""
    if setting in _CHILD_OUT:
        return _CHILD_OUT[setting]
    if _CHILD_FAILED:
        pytest.fail("the child process %r ended abnormally: no further child is started" % _CHILD_FAILED[0])
    extra, names, seconds = CHILDREN[setting]
    out = tmp_path_factory.mktemp("wx_" + setting)
    env = dict(os.environ, ABC_DIAG="1", **extra)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_wx_worker.py"), str(out)] + names, capture_output=True, text=True,
                           timeout=seconds, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _CHILD_FAILED.append(setting)
        pytest.fail("the child process %r ran into its time limit: %s" % (setting, str(e.stdout)[-2000:]))
    if p.returncode != 0:
        _CHILD_FAILED.append(setting)
        pytest.fail("the child process %r ended with %d: %s %s" % (setting, p.returncode, p.stdout[-1500:], p.stderr[-3000:]))
    _CHILD_OUT[setting] = out
    return out


def _run(name, setting, gpu_ctx, tmp_path_factory):
    """the reduction of a case under a setting: in this process ("asis") or from the setting's child"""
    key = (name, setting)
    if key not in _RUNS:
        if setting == "asis":
            X, Y, obs, A = W.make_data(name)
            _RUNS[key] = WXR.run_reduction(gpu_ctx, X, Y, obs, A, 0.5, record=True, both=True)
        else:
            with open(os.path.join(str(_child(setting, tmp_path_factory)), name + ".pkl"), "rb") as fh:
                _RUNS[key] = pickle.load(fh)
    return _RUNS[key]


def _ref(name, run, oracle):
    """the references of a case, computed once on the model of the first run that asks; every later run has the same model"""
    if name not in _REF:
        X, Y, obs, A = W.make_data(name)
        ref = WXR.reference(oracle, X, Y, run["m0"], A, run["ntrain"])
        assert np.array_equal(ref["optima"][ref["seg_j"]], ref["astar"]), name          # (same argmin PRESS on both sides)
        _REF[name] = (run["m0"].tobytes(), ref)
    assert run["m0"].tobytes() == _REF[name][0], name
    return _REF[name][1]


def _sweeps(name, run, setting):
    """the sweep instantiations of the run by the dispatch model, from the levels the record shows; the model's choice of bins
    is held against the record's on the way"""
    from abcsmc_amd import _lib
    N, M, P, A = W.CASES[name][:4]
    nv = N - run["ntrain"]
    rec = run["rec"]
    fine = []
    for k in range(1, _lib.WX_REC_LEVELS):
        at = [r for r in rec if r["n_levels"] > k]
        if not at:
            break
        bins = {r["levels"][k][0] for r in at}
        assert bins == {D.pick_bins(len(at), nv)}, (name, setting, k, bins, len(at))
        if k == 2:
            assert D.second_fine_level(at[0]["levels"][2][0], at[0]["levels"][1][0], len(at)), (name, setting)
        fine.append((bins.pop(), len(at)))
    n_exact = sum(r["w_taken"] for r in rec) if run["path"] == _lib.WX_PATH_CASCADE else 0
    return D.sweeps_of_run(nv, P, A, fine, n_exact, CAP_KB[setting])


def _check(name, setting, run, oracle, sorted_path):
    from abcsmc_amd import _lib
    ref = _ref(name, run, oracle)
    assert run["m1"].tobytes() == run["m1_off"].tobytes(), (name, setting)        # the same call with the record off: the same bytes
    out = WXR.check_record(run["path"], run["rec"], ref, run["m1"], W.CASES[name][2], sorted_path=sorted_path, label="%s/%s" % (name, setting))
    assert not ref["near"] and out["left_out"] == 0, (name, ref["near"])          # no reference p within 1e-9 of 0.1 for these seeds
    print("wilcoxon %s/%s: %d tests, path %d, %d sums taken, %d verdicts by the bounds, levels %s, %d of %d successive intervals nested"
          % (name, setting, len(run["rec"]), run["path"], out["taken"], out["settled"], sorted(out["levels"].items()), out["nested"], out["pairs"]))
    return ref, out


@pytest.mark.parametrize("name", list(W.CASES_SORTED))
def test_sorted_path(gpu_ctx, oracle, tmp_path_factory, name):
    """k_wx_diffs, the two radix sorts and k_wx_ranksum: nz and 2 W of every test equal the references as integers"""
    from abcsmc_amd import _lib
    N, M, P, A = W.CASES[name][:4]
    assert D.path(N - N // 2, P, A) == "sorted"
    run = _run(name, "asis", gpu_ctx, tmp_path_factory)
    assert run["path"] == _lib.WX_PATH_SORTED
    ref, out = _check(name, "asis", run, oracle, True)
    assert out["taken"] == len(run["rec"]) > 0
    if W.CASES[name][4] == "zeros":
        assert np.all(ref["m"] <= N - N // 2 - 40)                                 # the case does hold zero differences


@pytest.mark.parametrize("setting", ["asis", "forced", "forced_capped"])
@pytest.mark.parametrize("name", list(W.CASES_CASCADE))
def test_cascade_small(gpu_ctx, oracle, tmp_path_factory, name, setting):
    """16 384 validation rows and just above: as it is (bounds on every test), with every test forced through the exact step
    (2 W of every test; the MODE 2 sweeps), and forced with the counter buffer capped (a fine level in several batches)"""
    from abcsmc_amd import _lib
    N, M, P, A = W.CASES[name][:4]
    assert D.path(N - N // 2, P, A) == "cascade"
    run = _run(name, setting, gpu_ctx, tmp_path_factory)
    assert run["path"] == _lib.WX_PATH_CASCADE
    ref, out = _check(name, setting, run, oracle, False)
    assert all(r["n_levels"] >= 1 for r in run["rec"])
    if W.CASES[name][4] == "zeros":
        assert np.all(ref["m"] <= N - N // 2 - 40)
    inst, nbatch = _sweeps(name, run, setting)
    assert (D.am_of(A), 1, 0) in inst
    if setting != "asis":
        passed = set()                   # (a test without a non-zero difference passes at level 0; nothing behind it is looked at)
        for r, m in zip(run["rec"], ref["m"]):
            assert (r["verdict"], r["w_taken"]) == ((1, 0) if m == 0 else (2, 0 if r["response"] in passed else 1)), r
            if m == 0:
                passed.add(r["response"])
        assert (D.am_of(A), D.rkeys(A), 2) in inst and (D.am_of(A), 1, 1) in inst
        if name == "c8_copies" and setting == "forced":
            # k_wx_ranks_big: every test of the exact step has more distinct keys than the step has bins, so a bin with two values or
            # more exists, and every value fills a sub-bin beyond what k_wx_ranks walks (tests/_wx_worker.py)
            X, Y, obs, _ = W.make_data(name)
            ref_d = WXR.reference(oracle, X, Y, run["m0"], A, run["ntrain"], want_d=True)
            for r, d in zip(run["rec"], ref_d["d"]):
                if r["w_taken"]:
                    u, cnt = np.unique(np.abs(d[d != 0.0]), return_counts=True)
                    assert u.size > D.nbcap(N - N // 2) and D.WX_WALK < cnt.min() and cnt.max() <= D.WX_CAP, (r, u.size, cnt.min())
    if setting == "forced_capped" and name in ("c8_plain", "c32_plain"):       # (55 and ~30 open tests: more than one group of 29 / 16)
        assert nbatch[1] > 1, nbatch


@pytest.mark.parametrize("setting", ["forced", "capped"])
@pytest.mark.parametrize("name,want", [("a8_r2", (8, 2, 1)), ("a8_r4", (8, 4, 1)), ("a16_r2", (16, 2, 1))])
def test_cascade_many_tests(gpu_ctx, oracle, tmp_path_factory, name, want, setting):
    """65 537 validation rows with 112 .. 224 tests: forced, the fine level has enough groups of tests for two and four rows per
    thread; capped (and otherwise as it is), level 0 of 224 possible tests goes in two batches"""
    from abcsmc_amd import _lib
    run = _run(name, setting, gpu_ctx, tmp_path_factory)
    assert run["path"] == _lib.WX_PATH_CASCADE
    ref, out = _check(name, setting, run, oracle, False)
    inst, nbatch = _sweeps(name, run, setting)
    if setting == "forced":
        assert want in inst, (inst, nbatch)
        assert out["taken"] == len(run["rec"])
    elif name == "a8_r4":
        assert nbatch[0] == 2, nbatch


@pytest.mark.parametrize("name", list(W.CASES_OUTGROW))
def test_cascade_repeats_on_the_sorted_path(gpu_ctx, oracle, tmp_path_factory, name):
    """tie groups above 16 384 keys outgrow a bin of the exact step: the record says that the reduction was repeated on the
    sorted path and carries that path's sums, all of them; the bounds of the cascade's levels stay in it.  With one distinct
    validation row every interval is a point, of either sign."""
    from abcsmc_amd import _lib
    run = _run(name, "forced", gpu_ctx, tmp_path_factory)
    assert run["path"] == _lib.WX_PATH_CASCADE_THEN_SORTED
    ref, out = _check(name, "forced", run, oracle, True)
    assert out["taken"] == len(run["rec"]) > 0 and all(r["n_levels"] >= 1 for r in run["rec"])
    asis = _run(name, "asis", gpu_ctx, tmp_path_factory)                           # one sign per tie group: the bounds are points
    assert asis["path"] == _lib.WX_PATH_CASCADE
    ref, out2 = _check(name, "asis", asis, oracle, False)
    # one or two distinct keys per test: every interval EQUALS the bounds of one of the two ways to bin them (exact, also against a
    # bound that is too loose); most are points, and for two rows a positive key is among them
    X, Y, obs, A = W.make_data(name)
    ref_d = WXR.reference(oracle, X, Y, run["m0"], A, run["ntrain"], want_d=True)
    pts = WXR.check_few_keys(run["rec"], ref_d, 2) + WXR.check_few_keys(asis["rec"], ref_d, 2)
    if name == "c8_one_row":         # (the optimum has the smallest error on the one row there is: every difference is negative)
        assert out["points"] == 2 * len(ref["m"]) and out2["points"] == len(ref["m"]) and pts == 0
    else:
        assert pts >= 3, pts


@pytest.mark.parametrize("name,want", [("l8", (8, 2, 0)), ("l16", (16, 2, 0))])
def test_large_level0_two_rows_per_thread(gpu_ctx, oracle, tmp_path_factory, name, want):
    """391 169 validation rows: the smallest count at which level 0 runs two rows per thread with one group of tests"""
    N, M, P, A = W.CASES[name][:4]
    nv = N - N // 2
    assert nv == 191 * 2048 + 1
    assert D.batches(nv, A, P * (A - 1), D.WX_NC0, 0, D.bc_bytes(nv, P * (A - 1)))[0]["R"] == 2
    assert D.batches(nv - 1, A, P * (A - 1), D.WX_NC0, 0, D.bc_bytes(nv - 1, P * (A - 1)))[0]["R"] == 1
    run = _run(name, "asis", gpu_ctx, tmp_path_factory)
    _RUNS.pop((name, "asis"))                                                      # (nothing else reads it)
    ref, out = _check(name, "asis", run, oracle, False)
    assert want in _sweeps(name, run, "asis")[0]
    _REF.pop(name)


def _fused_generation(gpu_ctx, X, Y, obs, A, K=512, Kp=512, Nn=1024, seed=4242):
    """one fused generation under the Wilcoxon rule on (X, Y) with the record on -> (largest count, path, record): uniform priors
    over each parameter's range, a previous set drawn from the rows"""
    import torch
    from abcsmc_amd import _lib, abcutil, device
    N, M = X.shape
    P = Y.shape[1]
    spec = [(_lib.PRIOR_UNIF_REAL, float(Y[:, j].min() - Y[:, j].std()), float(Y[:, j].max() + Y[:, j].std())) for j in range(P)]
    th_prev = np.asfortranarray(Y.mean(0) + 0.5 * (Y[:Kp] - Y.mean(0)))
    w_prev, dv_prev = np.full(Kp, 1.0 / Kp), 2.0 * th_prev.var(axis=0, ddof=1)
    dev = "cuda:0"
    gen = device.Generation(N, M, P, K, Kp, Nn, train_frac=0.5, max_comp=A, rule=_lib.RULE_WILCOXON, multivariate=True, device=dev)
    gpu_ctx.set_wx_record(True)
    try:
        gen.run(device.colmajor(X, dev), device.colmajor(Y, dev), device.colmajor(obs, dev), device.priors_to_device(_lib.make_priors(spec), dev),
                abcutil.rng(seed), device.colmajor(th_prev, dev), device.colmajor(w_prev, dev), device.colmajor(dv_prev, dev))
        torch.cuda.synchronize()
        path, rec = gpu_ctx.wx_last_record()
    finally:
        gpu_ctx.set_wx_record(False)
    return int(gen.ncomp.value), path, rec


@pytest.mark.parametrize("name", ["c8_plain", "c16_plain", "c32_plain"])
def test_fused_generation_largest_count_first(gpu_ctx, oracle, tmp_path_factory, name):
    """One fused generation under the Wilcoxon rule (the largest count first: the picked responses' tests, then -- where none of
    them keeps its optimum -- the others'; tests left open as not needed): the record of its reduction against the references
    on the same model, fitted again through the staged entry points from the same statistics.  Tests the cascade never looked at
    or left open are exempt from the comparison of W, none from containment."""
    from abcsmc_amd import _lib
    N, M, P, A = W.CASES[name][:4]
    X, Y, obs, A = W.make_data(name)
    ncomp, path, rec = _fused_generation(gpu_ctx, X, Y, obs, A)
    assert path == _lib.WX_PATH_CASCADE and D.first_r(P, A, True) > 0
    plain = _run(name, "asis", gpu_ctx, tmp_path_factory)
    ref = _ref(name, plain, oracle)
    out = WXR.check_record(path, rec, ref, None, P, sorted_path=False, plain=False, label="fused/" + name)
    assert not ref["near"] and out["left_out"] == 0
    verdicts = [r["verdict"] for r in rec]
    print("fused generation %s: %d tests, verdicts 0/1/2/3: %s, %d sums taken, %d never looked at, levels %s"
          % (name, len(rec), [verdicts.count(v) for v in range(4)], out["taken"], sum(r["n_levels"] == 0 for r in rec), sorted(out["levels"].items())))
    assert all(r["n_levels"] >= 1 for r in rec if r["verdict"] != 2)
    if name == "c8_plain":           # a picked response keeps its optimum: the other responses' tests are never looked at
        assert any(r["n_levels"] == 0 for r in rec)
    else:                            # none does: level 0 over the other responses too, open tests nobody needs left open
        assert all(r["n_levels"] >= 1 for r in rec) and 3 in verdicts and 1 in verdicts
    # the generation used the largest count, and that is the plain reduction's
    L = len(plain["m1"]) - 8
    assert ncomp == int(plain["m1"][0]) == int(plain["m1"][L - P:L].max())


def test_every_reachable_sweep_instantiation_is_reached(gpu_ctx, oracle, tmp_path_factory):
    """the union over the cases above is every k_wx_sweep instantiation a run can launch but <8, 4, 0>, which needs 196 609
    validation rows even with 4 groups of tests and is reached at 5e6 rows by test_gpu_parity.py's binned-path case"""
    got = set()
    for setting, names in [("asis", list(W.CASES_CASCADE))] + [(s, CHILDREN[s][1]) for s in ("forced", "forced_capped", "capped")]:
        for name in names:
            if name in W.CASES_OUTGROW:
                continue
            got |= _sweeps(name, _run(name, setting, gpu_ctx, tmp_path_factory), setting)[0]
    for name, want in (("l8", (8, 2, 0)), ("l16", (16, 2, 0))):                   # (their runs are checked above; here the model alone)
        N, M, P, A = W.CASES[name][:4]
        nv = N - N // 2
        got |= {D.sweep_instantiation(A, g["R"], 0) for g in D.batches(nv, A, P * (A - 1), D.WX_NC0, 0, D.bc_bytes(nv, P * (A - 1)))}
    assert got == D.reachable() - {(8, 4, 0)}, (sorted(D.reachable() - got), sorted(got - D.reachable()))
    assert D.batches(5_000_000, 4, 6, D.WX_NC0, 0, D.bc_bytes(5_000_000, 6))[0]["R"] == 4
