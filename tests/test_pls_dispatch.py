"""CPU checks of tests/_pls_dispatch.py, the tests' copy of the model fit's kernel choice (pls.hip: launch_pls_model): the
instantiations it can reach are exactly the launch sites of launch_pls_model, so the copy and the source cannot drift apart
unseen, and the decisions on both sides of every threshold are pinned."""
import os
import re

from _pls_dispatch import LDS_LIMIT, fit_plan, lds_fit16_doubles, lds_fit_doubles, reachable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch_table():
    src = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "pls.hip")).read()
    body = src[src.index("int launch_pls_model("):]
    body = body[:body.index("#undef PLS_LAUNCH\n")]
    nb_def = re.search(r"#define PLS_LAUNCH_NB\(NW_\)(.*?)while \(0\)", body, re.S).group(1)
    nb_values = [int(v) for v in re.findall(r"PLS_LAUNCH\(NW_,\s*false,\s*(\d+)\)", nb_def)]
    assert sorted(nb_values) == [0, 1, 2], nb_def
    calls = re.sub(r"#define[^\n]*(\\\n[^\n]*)*", "", body)              # the launch sites, not the macro bodies
    out = set()
    for nw, gm, nb in re.findall(r"PLS_LAUNCH\((\d+),\s*(true|false),\s*(\d+)\)", calls):
        out.add(("fit", int(nw), gm == "true", int(nb)))
    for nw in re.findall(r"PLS_LAUNCH_NB\((\d+)\)", calls):
        out |= {("fit", int(nw), False, nb) for nb in nb_values}
    for nw, nb in re.findall(r"FIT16_LAUNCH\((\d+),\s*(\d+)\)", calls):
        out.add(("fit16", int(nw), int(nb)))
    return out


def test_mirror_reaches_exactly_the_launch_sites():
    table = _launch_table()
    assert len(table) == 15, sorted(table)
    mirror = reachable()
    assert mirror == table, ("in the mirror only: %s; in pls.hip only: %s" % (sorted(mirror - table), sorted(table - mirror)))


def _k(M, P, A):
    return fit_plan(M, P, A)["kernel"]


def test_metric_thresholds():
    # 16 / 17 metrics: one wavefront, then four waves (or the latency-tuned fit)
    assert _k(16, 5, 4) == ("fit", 1, False, 1) and _k(17, 5, 4) == ("fit16", 4, 1)
    assert _k(16, 1, 4) == ("fit", 1, False, 1) and _k(17, 1, 4) == ("fit", 4, False, 1)
    assert _k(16, 40, 4) == ("fit", 1, False, 0) and _k(17, 40, 4) == ("fit", 4, False, 0)
    # 64 / 65: four waves, then eight; X'X in LDS, then in registers
    assert fit_plan(64, 5, 8) == {"kernel": ("fit16", 4, 1), "fold_z": False, "eig": "square1", "xx": "lds", "press": "entry",
                                  "q8": False}
    assert fit_plan(65, 5, 8) == {"kernel": ("fit16", 8, 1), "fold_z": False, "eig": "square1", "xx": "reg", "press": "entry",
                                  "q8": False}
    assert fit_plan(64, 40, 8)["kernel"] == ("fit", 4, False, 0) and fit_plan(64, 40, 8)["xx"] == "lds"
    assert fit_plan(65, 40, 8)["kernel"] == ("fit", 8, False, 0) and fit_plan(65, 40, 8)["xx"] == "reg"
    # 128 / 129: X'X in registers, then from global memory (both families)
    assert fit_plan(128, 5, 8)["xx"] == "reg" and fit_plan(129, 5, 8)["xx"] == "global"
    assert fit_plan(128, 1, 8)["xx"] == "reg" and fit_plan(129, 1, 8)["xx"] == "global"
    assert fit_plan(128, 1, 8)["kernel"] == fit_plan(129, 1, 8)["kernel"] == ("fit", 8, False, 1)
    # fit16 on two blocks per side never keeps X'X in registers (the eigen matrices take them)
    assert fit_plan(100, 20, 8) == {"kernel": ("fit16", 8, 2), "fold_z": False, "eig": "square2", "xx": "global",
                                    "press": "entry", "q8": False}


def test_response_thresholds():
    # 1 / 2 responses: w = XY, then the eigenvector; the latency-tuned fit from 2
    assert fit_plan(20, 1, 4)["kernel"] == ("fit", 4, False, 1) and fit_plan(20, 1, 4)["eig"] is None
    assert fit_plan(20, 2, 4)["kernel"] == ("fit16", 4, 1) and fit_plan(20, 2, 4)["eig"] == "square1"
    # 16 / 17: one 16 x 16 block per side, then two
    assert _k(20, 16, 4) == ("fit16", 4, 1) and _k(20, 17, 4) == ("fit16", 4, 2)
    assert _k(10, 16, 4) == ("fit", 1, False, 1) and _k(10, 17, 4) == ("fit", 1, False, 2)
    # 32 / 33: the latency-tuned fit stops, 4 x 4 blocks
    assert _k(20, 32, 4) == ("fit16", 4, 2) and fit_plan(20, 33, 4)["kernel"] == ("fit", 4, False, 0)
    assert fit_plan(20, 33, 4)["eig"] == "square4"
    # 64 / 65: the register-resident squaring, then the memory-resident one
    assert fit_plan(10, 64, 4)["eig"] == "square4" and fit_plan(10, 65, 4)["eig"] == "generic"
    assert fit_plan(10, 65, 4)["kernel"] == ("fit", 1, False, 0)
    # wide sets with 17..64 responses run the 4 x 4 blocks in global memory
    assert fit_plan(63, 63, 32) == {"kernel": ("fit", 8, True, 0), "fold_z": False, "eig": "square4", "xx": "lds",
                                    "press": "gemm", "q8": False}


def test_fold_and_press_thresholds():
    # k_zstats folded into k_pls_fit16 while M (M + P) <= 4096
    assert 60 * 68 == 4080 and fit_plan(60, 8, 4)["fold_z"] and not fit_plan(60, 9, 4)["fold_z"]
    assert fit_plan(60, 9, 4)["kernel"] == ("fit16", 4, 1)
    assert not fit_plan(16, 5, 4)["fold_z"]                       # (k_pls_fit never folds)
    # the PRESS contractions on the matrix pipe from A M >= 1024
    assert fit_plan(64, 5, 16)["press"] == "gemm" and fit_plan(64, 5, 15)["press"] == "entry"
    assert fit_plan(32, 5, 32)["press"] == "gemm" and fit_plan(31, 5, 31)["press"] == "entry"
    # eight threads per response for q = XY'r / tt: eight waves, M > 64, 4 M >= 8 P
    assert fit_plan(65, 1, 4)["q8"] and fit_plan(66, 33, 4)["q8"] and not fit_plan(65, 33, 4)["q8"]
    assert not fit_plan(64, 1, 4)["q8"]


def test_lds_limits():
    # k_pls_fit16's LDS: 59 components of (63, 15) fit, 60 do not (then k_pls_fit on four waves)
    assert lds_fit16_doubles(63, 15, 59) * 8 <= LDS_LIMIT < lds_fit16_doubles(63, 15, 60) * 8
    assert lds_fit16_doubles(63, 15, 59) == 6572 + 172 * 59 + 59 * 59
    assert _k(63, 15, 59) == ("fit16", 4, 1) and _k(63, 15, 60) == ("fit", 4, False, 1)
    # k_pls_fit's work arrays: 77 components of (100, 16) in LDS, 78 in global memory
    assert lds_fit_doubles(100, 16, 77) * 8 <= LDS_LIMIT < lds_fit_doubles(100, 16, 78) * 8
    assert lds_fit_doubles(100, 16, 77) == 4992 + 201 * 77
    assert _k(100, 16, 77) == ("fit", 8, False, 1) and _k(100, 16, 78) == ("fit", 8, True, 1)
    assert fit_plan(100, 16, 78)["xx"] == "global"                # (no registers for X'X in the global-memory mode)
