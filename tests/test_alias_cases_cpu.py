"""CPU side of the device alias build's branch tests: the step-map algebra (abcsmc_amd/csrc/alias_maps.h) against brute force,
and the build's exact-integer model (scripts/alias_scan_proto.py) against the oracle on the structured weight vectors of
tests/_alias_cases.py -- the model's verdicts are what tests/test_gpu_alias_branches.py holds the kernels' fallbacks to."""
import os
import subprocess

import numpy as np
import pytest

import _alias_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan_ubsan"])
def test_alias_maps_probe(tmp_path, flags):
    """rne_map / rapply, inv_min, compose, to_grid / from_grid as the kernels compile them, on the host against brute force in
    __int128 (tests/cxx/alias_maps_probe.cpp): plain, and under the address and undefined-behaviour sanitizers (a stand-alone
    host program: the shifts by k + 1 and -sh, the ceilings of negative operands, the 128-bit wrap of shl)"""
    exe = str(tmp_path / "alias_maps_probe")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cxx", "alias_maps_probe.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 1_000_000 and out.stderr == ""


def _grid():
    return [(kind, K) for kind in ac.KINDS for K in ac.EDGE_SIZES if not (kind in ac.FULL_KINDS and K < 4)]


@pytest.mark.parametrize("kind", ac.KINDS)
def test_model_builds_the_oracles_table(oracle, kind):
    """every chain shape at every block edge: where the model's speculation verifies, its table is the oracle's
    gsl_ran_discrete_preproc bit for bit (F compared after the KNUTH_CONVENTION map, as abc_alias_table applies it); the verdict
    does not depend on the order of the approximate prefix sums; the cells that fall back are exactly the listed ones"""
    for k2, K in _grid() + [(k, K) for k in ac.RESAMPLE_KINDS for K in ac.RESAMPLE_SIZES]:
        if k2 != kind:
            continue
        w, m = ac.cell(kind, K)
        assert w.size == K and np.all(np.isfinite(w)) and np.all(w >= 0) and w.sum() > 0
        assert m["on_device"] is not None, "verdict depends on the summation order: re-seed (%s, %d) in RESEED" % (kind, K)
        assert m["on_device"] == (not ac.expect_host(kind, K)), (kind, K, m["reason"])
        if kind in ac.FULL_KINDS:
            assert m["reason"].startswith("expected no demotion"), (kind, K, m["reason"])
        elif not m["on_device"]:
            assert m["reason"].startswith(ac.EXPECT_HOST[(kind, K)].split(":")[0]), (kind, K, m["reason"])
        if m["on_device"]:
            oF, oA = oracle.discrete_preproc(w)
            assert np.array_equal(m["A"], oA), (kind, K)
            assert np.array_equal(m["F"].view(np.uint64), oF.view(np.uint64)), (kind, K)


def test_fallback_share_and_shapes():
    """outside exactly_full the model may send at most one cell in twenty to the host; and the generators give the shapes their
    names promise (so that a change to them cannot quietly turn the grid into random vectors)"""
    plain = [(kind, K) for kind, K in _grid() if kind not in ac.FULL_KINDS]
    assert 20 * sum(c in ac.EXPECT_HOST for c in plain) <= len(plain)
    K = 1025
    mean_of = lambda w: w.sum() / w.size
    w = ac.weights("ascending", K); assert np.all(np.diff(w) >= 0)
    w = ac.weights("descending", K); assert np.all(np.diff(w) <= 0)
    for kind, at in (("one_big", K // 3), ("one_big_first", 0), ("one_big_last", K - 1)):
        w = ac.weights(kind, K); assert np.flatnonzero(w >= mean_of(w)).tolist() == [at]
    w = ac.weights("one_hot", K); assert np.count_nonzero(w) == 1
    w = ac.weights("alternating", K); assert np.array_equal(w >= mean_of(w), np.arange(K) % 2 == 1)
    w = ac.weights("smalls_then_bigs", K); assert np.array_equal(w >= mean_of(w), np.arange(K) >= K // 2)
    w = ac.weights("bigs_then_smalls", K); assert np.array_equal(w >= mean_of(w), np.arange(K) < K // 2)
    w = ac.weights("mostly_zero", K); assert 0.89 * K <= np.count_nonzero(w == 0) <= 0.91 * K
    w = ac.weights("zero_head", K); assert np.all(w[:K // 3] == 0) and np.all(w[K // 3:] > 0)
    w = ac.weights("zero_tail", K); assert np.all(w[K - K // 3:] == 0) and np.all(w[:K - K // 3] > 0)
    w = ac.weights("one_small", K); assert np.count_nonzero(w < 1) == 1
    assert ac.weights("exactly_full", 4).tolist() == [1.0, 2.0, 2.0, 3.0]
    for kind in ac.FULL_KINDS:
        w = ac.weights(kind, K); assert w.sum() == 2 * K and sorted(set(w.tolist())) == [1.0, 2.0, 3.0]
    # handover_chain: (nearly) every big is demoted after about one small -- the chain has as many hand-overs as bigs
    _, m = ac.cell("handover_chain", K)
    assert m["nsteps"] == K - 1 and abs(m["ns"] - K // 2) <= 1
    # the two-valued vectors of the GPU test put ns, nb and nsteps where their labels say (nsteps from the model), K elsewhere
    for elems in (2, 4):
        B = 256 * elems
        cases = ac.block_edge_cases(elems)
        assert sorted(c[0] for c in cases) == sorted(["%s=%s" % (q, t) for q in ("ns", "nb", "nsteps") for t in ("B-1", "B", "B+1", "2B")])
        for label, w, m in cases:
            q, t = label.split("=")
            assert m[q] == {"B-1": B - 1, "B": B, "B+1": B + 1, "2B": 2 * B}[t], (elems, label, m["ns"], m["nb"], m["nsteps"])
            assert m["on_device"] is True, (elems, label, m["reason"])
            assert q == "nsteps" or min(w.size % B, B - w.size % B) > 1, (elems, label, w.size)
