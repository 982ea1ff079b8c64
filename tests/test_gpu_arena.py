"""Every entry point held to its own arena reservation, on a fresh and on a grown arena, poisoned and not.

The catalogue of tests/_arena_cases.py runs in two child processes (tests/_arena_worker.py), one after the other: the first as the
environment is, the second under ABC_WS_POISON=ff (the library reads the switch once, so it needs its own process; ABC_DIAG=1 comes
from conftest.py).  Each child runs every case on one warm context, grown to the largest reservation first and full of another
call's data, and on a fresh context of its own.  That makes four runs of every case, and per case:

  (a) the fresh context's return code is 0: ABC_ERR_NOMEM there is a bound that under-counts;
  (b) peak <= asked <= reserved (abc_ws_info) on the fresh and on the warm context: the bound is the library's own promise, so the
      cap has no margin, and on the warm context it catches the under-count a grown arena would absorb;
  (c) every output has the same bytes in all four runs (NaNs and signed zeros count): nothing is read that this call did not write;
  (d) every path counter is the same in all four runs: no path depends on what the arena held or how large it was;
  (e) the largest block the row states is at least a quarter of what the entry asked for on the fresh context ("block" rows only):
      this judges the row, not the library, and a row that misses it gets another shape.

The references of (c) are the other three runs of the same library; the numerics of every entry are held to their own references
elsewhere.  The second child is not started when the first did not exit 0.

Time limits: the first clean run of the unpoisoned child took 9.0 s on an MI355X (interpreter start, inputs and the two passes over
the 120 rows, which themselves take about a second each; the poisoned child 8.8 s, the whole file 20 s); each child gets three times
that."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _arena_cases as AC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 9            # the first clean run of the unpoisoned child
TIMEOUT = 3 * CHILD_SECONDS
RUNS = [(child, mode) for child in ("plain", "poison") for mode in ("warm", "fresh")]


def _child(out, poison):
    env = dict(os.environ)
    env.pop("ABC_WS_POISON", None)
    if poison:
        env["ABC_WS_POISON"] = "ff"
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_arena_worker.py"), out], capture_output=True, text=True,
                          timeout=TIMEOUT, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(child, mode, case): {field: array}} of the two children"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("arena")
    rec = {}
    for child in ("plain", "poison"):
        out = str(d / (child + ".npz"))
        t0 = time.perf_counter()
        p = _child(out, child == "poison")
        print("the %s child took %.1f s (limit %d s)" % (child, time.perf_counter() - t0, TIMEOUT))
        # (a child that fails is a finding of its last case: the poisoned one is then not started on the same device)
        assert p.returncode == 0, "the %s child ended with %d; its last lines:\n%s\n%s" % (child, p.returncode, p.stdout[-2000:],
                                                                                         p.stderr[-3000:])
        with np.load(out) as z:
            for key in z.files:
                mode, name, field = key.split("|", 2)
                rec.setdefault((child, mode, name), {})[field] = z[key]
    return rec


CASES = sorted(AC.CASES)


def _say(r):
    return "rc %d %s (reserved, asked, peak) = %s" % (int(r["rc"]), str(r["err"]), r["info"].tolist())


@pytest.mark.parametrize("name", CASES)
def test_first_call_on_a_fresh_context_returns_ok(runs, name):
    for child in ("plain", "poison"):
        r = runs[(child, "fresh", name)]
        assert int(r["rc"]) == 0, (child, _say(r))


@pytest.mark.parametrize("name", CASES)
def test_peak_within_asked_within_reserved(runs, name):
    for child, mode in RUNS:
        r = runs[(child, mode, name)]
        reserved, asked, peak = (int(v) for v in r["info"])
        print(child, mode, name, "reserved %d asked %d peak %d" % (reserved, asked, peak))
        assert int(r["rc"]) == 0, (child, mode, _say(r))
        assert peak <= asked <= reserved, (child, mode, _say(r))


def _fields(r, counters):
    return {k: v for k, v in r.items() if k.startswith("out:") and k.startswith("out:counter/") == counters}


def _same_in_all_runs(runs, name, counters):
    ref = _fields(runs[("plain", "fresh", name)], counters)
    assert ref, "the row returns nothing to compare"
    for child, mode in RUNS:
        r = runs[(child, mode, name)]
        assert int(r["rc"]) == 0, (child, mode, _say(r))
        got = _fields(r, counters)
        assert sorted(got) == sorted(ref), (child, mode, sorted(set(got) ^ set(ref)))
        for k in ref:
            a, b = np.ascontiguousarray(ref[k]), np.ascontiguousarray(got[k])
            assert a.dtype == b.dtype and a.shape == b.shape, (child, mode, k)
            same = np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))
            assert same, "%s differs between plain/fresh and %s/%s: %s" % (k, child, mode, "" if a.size > 16 else (a, b))


@pytest.mark.parametrize("name", CASES)
def test_outputs_have_the_same_bytes_in_all_four_runs(runs, name):
    _same_in_all_runs(runs, name, counters=False)


@pytest.mark.parametrize("name", CASES)
def test_path_counters_agree_in_all_four_runs(runs, name):
    _same_in_all_runs(runs, name, counters=True)


@pytest.mark.parametrize("name", [n for n in CASES if AC.CASES[n].klass == "block"])
def test_stated_block_is_a_quarter_of_the_reservation(runs, name):
    r = runs[("plain", "fresh", name)]
    asked = int(r["info"][1])
    dom = AC.CASES[name].dominant
    print(name, "largest stated block %d, asked %d (%.2f)" % (dom, asked, dom / max(asked, 1)))
    assert int(r["rc"]) == 0, _say(r)
    assert 4 * dom >= asked, "largest stated block %d of asked %d: give the row another shape" % (dom, asked)
