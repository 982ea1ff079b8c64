"""CPU checks of tests/_wx_dispatch.py, the tests' copy of the host decisions of wilcoxon.hip: the constants and thresholds are
read out of the source text, the k_wx_sweep instantiations out of the launch macros, so the copy and the source cannot drift
apart unseen; the decisions on both sides of every threshold are pinned."""
import os
import re

import _wx_dispatch as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "wilcoxon.hip")).read()


def _const(name):
    m = re.search(r"constexpr\s+(?:int|size_t)\s+%s\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*;" % name, SRC)
    assert m, name                                                  # (a literal, or literal << literal)
    return int(m.group(1)) << int(m.group(2) or 0)


def _body(start, end):
    a = SRC.index(start)
    return SRC[a:SRC.index(end, a)]


def test_constants_are_the_source_s():
    for name in ("WX_T", "WX_NC0", "WX_CSH", "WX_LDS", "WX_NBFMAX", "WX_FIRST_MAX", "MAXSEG", "WX_CAP", "WX_CAP_S", "WX_NS", "WX_WALK", "WX_PK"):
        assert getattr(D, name) == _const(name), name
    assert "static_assert(WX_NC0 == 3 * 64" in SRC


def test_thresholds_are_the_source_s():
    applies = _body("bool abc_wx_cascade_applies", "}")
    assert re.search(r"A >= 2 && A <= 32 && nv_total >= (\d+) && nv_total < \(\(size_t\)1 << 31\) && P \* \(A - 1\) <= MAXSEG", applies).group(1) == str(D.CASCADE_MIN_ROWS)
    one = _body("WxLevel wx_level_one(size_t nt, size_t A, int want, int NBX, size_t per_test_lds, size_t bc_bytes, int fixed_slots) {", "\nsize_t wx_bc_bytes")
    assert "g.G = (int)(((size_t)WX_LDS - 1024) / per_test_lds);" in one
    assert "const int rmax = A <= 8 ? 4 : (A <= 16 ? 2 : 1);" in one
    assert re.search(r"\* \(size_t\)g\.TG < (\d+)\) g\.R >>= 1;", one).group(1) == str(D.GROUPS_FLOOR)
    assert re.search(r"int rr_target = (\d+) / g\.TG;", one).group(1) == str(D.RUNS_TARGET)
    assert "const int limit = 65535 / (g.TT * g.R);" in one and "for (int it = 0; it < 8; it++)" in one
    assert "int fit = (int)(bc_bytes / ((size_t)rr_bytes * NBX * 4)) / g.G * g.G;" in one
    bc = _body("size_t wx_bc_bytes(size_t nv, size_t nseg_max) {", "\n}")
    assert "nseg_max * 2048 * 4 > (size_t)8 * WX_NBFMAX * 4" in bc and "size_t cap = (size_t)96 << 20;" in bc and "+ (1u << 20);" in bc
    assert D.BC_CAP == 96 << 20
    pick = _body("int wx_pick_bins(int nact, size_t nvt) {", "\n}")
    assert "126.0 * sqrt((double)nvt / 5.0e5)" in pick and "for (int nb = 16384; nb >= 1024; nb >>= 1)" in pick
    assert "if (nb > 1024 && (size_t)nb * 4 > nvt) continue;" in pick and "const double cost = passes + 1.5 * open * nact;" in pick
    assert "((size_t)nb * 4 + WX_NC0 * 4 + 7 * 4 + 16)" in pick
    assert "size_t xb = ((size_t)1 << 25) / (nvt ? nvt : 1);" in SRC and "return xb < 1 ? 1 : (xb > 8 ? 8 : (int)xb);" in SRC
    assert "const size_t t = (nvt + 3499) / 3500; return (unsigned int)(t > 2048 ? t : 2048);" in SRC
    assert (D.XB_KEYS, D.TARGET_DIV, D.TARGET_MIN) == (1 << 25, 3500, 2048)
    assert "const size_t per_test = (size_t)NBX * 4 + (mode == 1 ? WX_NC0 * 4 : 0) + 7 * 4 + 16;" in SRC
    assert "const int rkeys = A <= 8 ? 4 : (A <= 16 ? 2 : 1);" in SRC
    assert "const int nbcap = (int)(nvt / target) + 2;" in SRC
    assert "first_r = 32 / (int)(A - 1);" in SRC and "first_r = first_r < 2 ? 2 : (first_r > 4 ? 4 : first_r);" in SRC
    assert "if (stop_at_max && P <= 1024 && A >= 2) {" in SRC and "if ((size_t)first_r >= P) first_r = 0;" in SRC
    assert "if (f == 1 && (NBX <= NBX_last || left > 32)) break;" in SRC
    # the score kernels: one helper, the power of two at or above A (the projection's rounding, project_plan.h) through one table
    # by its log2; the wide kernel above 32 components only -- which is the sorted path only (abc_wx_cascade_applies above)
    plan_h = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "project_plan.h")).read()
    kc = re.search(r"inline int abc_project_kc\(size_t A\) \{(.*?)\n\}", plan_h, re.S).group(1)
    assert "int KC = 1;\n    while (KC < (int)A) KC *= 2;\n    if (KC > 32) KC = (int)((A + 31) / 32) * 32;\n    return KC;" in kc
    assert "while (KC < (int)A)" not in SRC and "LAUNCH_SC" not in SRC
    table = re.search(r"static const WxScoresFn WX_SCORES\[6\] = \{(.*?)\};", SRC, re.S).group(1)
    assert [s.strip() for s in table.split(",")] == ["k_wx_scores<%d>" % v for v in (1, 2, 4, 8, 16, 32)]
    helper = _body("static void launch_wx_scores(", "\n}\n")
    assert "const int KC = abc_project_kc(A);\n    if (KC > 32)\n        hipLaunchKernelGGL(k_wx_scores_wide," in helper
    assert "    else\n        hipLaunchKernelGGL(WX_SCORES[__builtin_ctz((unsigned)KC)]," in helper and helper.count("LaunchKernelGGL(") == 2
    # both call sites go through it, and nothing else launches a score kernel
    assert len(re.findall(r"LaunchKernelGGL\(\(?(?:k_wx_scores|WX_SCORES)", SRC)) == 2
    assert len(re.findall(r"\blaunch_wx_scores\(ctx, ", SRC)) == 2
    assert "launch_wx_scores(ctx, X, ldx, row_test, nt, M, P, A, model, S, nt);" in _body("int launch_wilcoxon_sorted(", "\n}\n")
    assert "launch_wx_scores(ctx, X + took, ldx, row_test, nt - took, M, P, A, model, S + took, nt);" in _body("static void wx_scores(", "\n}\n")


def test_sweep_instantiations_are_the_launch_macros():
    sweep = _body("static void wx_sweep(", "#undef WX_GO")
    go = re.findall(r"WX_GO\((\d+), (\d+), (\d+)\)", sweep)
    assert all(tt == "1024" for _, _, tt in go)
    launch = _body("static void wx_launch_sweep(", "#undef WX_SW")
    modes = sorted(int(v) for v in re.findall(r"WX_SW\((\d)\)", launch))
    assert modes == [0, 1, 2] and "k_wx_sweep<AM, R, MODEV, TT>" in launch
    from_macros = {(int(am), int(r), m) for am, r, _ in go for m in modes}
    assert from_macros == D.instantiable() and len(from_macros) == 18
    # the branches of wx_sweep, as the copy takes them
    assert "if (A <= 8) { if (g.R == 4) WX_GO(8, 4, 1024); else if (g.R == 2) WX_GO(8, 2, 1024); else WX_GO(8, 1, 1024); }" in sweep
    assert "else if (A <= 16) { if (g.R == 2) WX_GO(16, 2, 1024); else WX_GO(16, 1, 1024); }" in sweep and "else WX_GO(32, 1, 1024);" in sweep
    # no other launch site of the kernel
    assert len(re.findall(r"hipLaunchKernelGGL\(\(k_wx_sweep<", SRC)) == 1
    assert D.reachable() < D.instantiable() and D.instantiable() - D.reachable() == {(8, 2, 2), (8, 1, 2), (16, 1, 2)}
    assert [D.sweep_instantiation(A, R, 1) for A, R in ((2, 4), (8, 2), (8, 1), (9, 2), (16, 1), (17, 1), (32, 1))] == \
        [(8, 4, 1), (8, 2, 1), (8, 1, 1), (16, 2, 1), (16, 1, 1), (32, 1, 1), (32, 1, 1)]


def test_path_thresholds():
    assert D.path(16383, 4, 8) == "sorted" and D.path(16384, 4, 8) == "cascade" and D.path(16384, 4, 33) == "sorted"
    assert D.path(16384, 4, 32) == "cascade" and D.path(16384, 4, 1) == "none" and D.path(0, 4, 8) == "none"
    assert D.path(1 << 31, 4, 8) == "sorted" and D.path((1 << 31) - 1, 4, 8) == "cascade"
    assert D.path(20000, 9362, 8) == "cascade" and D.path(20000, 9363, 8) == "sorted"       # 65534 / 65541 tests
    assert D.path(20000, 4, 8, force_sorted=True) == "sorted"
    assert [D.scores_kc(A) for A in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, "wide", "wide"]
    assert [D.rkeys(A) for A in (2, 8, 9, 16, 17, 32)] == [4, 4, 2, 2, 1, 1] == [D.rmax(A) for A in (2, 8, 9, 16, 17, 32)]
    assert [D.first_r(12, A, True) for A in (2, 8, 9, 12, 17, 32)] == [4, 4, 4, 2, 2, 2]
    assert D.first_r(4, 8, True) == 0 and D.first_r(5, 8, True) == 4 and D.first_r(12, 8, False) == 0 and D.first_r(1025, 8, True) == 0


def test_level_geometry():
    lvl0 = lambda nv, A, n, cap=None: D.batches(nv, A, n, D.WX_NC0, 0, D.bc_bytes(nv, n, cap))
    # a group of level 0: 180 tests (812 bytes each in 143 KB)
    assert D.per_test_lds(192, 0) == 812 and D.per_test_lds(1024, 1) == 4908 and D.per_test_lds(4096, 1) == 17196
    assert lvl0(16391, 8, 56) == [dict(R=1, tiles=17, G=56, TG=1, RR=17, tpw=1, nslots=56)]
    assert lvl0(16391, 8, 181)[0]["TG"] == 2 and lvl0(16391, 8, 180)[0]["TG"] == 1
    # rows per thread: halved while tiles x groups < 192
    assert lvl0(191 * 4096, 8, 14)[0]["R"] == 2 and lvl0(191 * 4096 + 1, 8, 14)[0]["R"] == 4
    assert lvl0(191 * 2048, 8, 14)[0]["R"] == 1 and lvl0(191 * 2048 + 1, 8, 14)[0]["R"] == 2
    assert lvl0(191 * 2048, 16, 30)[0]["R"] == 1 and lvl0(191 * 2048 + 1, 16, 30)[0]["R"] == 2 and lvl0(10 ** 7, 32, 30)[0]["R"] == 1
    # the 300 000-row cases of test_gpu_parity.py (150 000 validation rows, 112 / 120 tests): one group, 37 / 74 tiles -- one row per thread
    assert lvl0(150000, 8, 112)[0]["R"] == 1 and lvl0(150000, 16, 120)[0]["R"] == 1 and lvl0(100000, 24, 138)[0]["R"] == 1
    assert lvl0(5_000_000, 4, 6)[0] == dict(R=4, tiles=1221, G=6, TG=1, RR=245, tpw=5, nslots=6)
    # runs of tiles: a work-group's rows stay below 2^16
    g = lvl0(40_000_000, 8, 7 * 400)[0]
    assert g["tpw"] * D.WX_T * g["R"] <= 65535 and g["RR"] * g["tpw"] >= g["tiles"]
    # the counter buffer capped: whole groups of tests per batch
    assert [g["nslots"] for g in lvl0(65537, 8, 224, 9216)] == [180, 44] and [g["nslots"] for g in lvl0(65537, 8, 224)] == [224]
    fine = D.batches(16391, 8, 56, 1024, 1, D.bc_bytes(16391, 56, 1024))
    assert [g["nslots"] for g in fine] == [29, 27] and all(g["R"] == 1 for g in fine)
    # a cap below one group of tests (17 runs x 29 tests x 1024 bins x 4 bytes here) is refused, by the library as by the copy
    import pytest
    with pytest.raises(AssertionError, match="do not fit the counter buffer"):
        D.batches(16391, 8, 56, 1024, 1, D.bc_bytes(16391, 56, 64))
    assert "if ((size_t)g.RR * g.nslots * NBX * 4 > bc_bytes)\n" in SRC


def test_bins_and_the_exact_step():
    assert D.pick_bins(1, 16384) == 4096 and D.pick_bins(1, 16383) == 2048 and D.pick_bins(1, 8192) == 2048 and D.pick_bins(1, 8191) == 1024
    assert D.pick_bins(1, 65536) == 16384 and D.pick_bins(1, 65535) == 8192
    assert D.pick_bins(56, 16391) == 1024 and D.pick_bins(112, 65537) == 2048 and D.pick_bins(10, 5_000_000) == 4096
    assert [D.xb(n) for n in (0, 1, 1 << 22, (1 << 22) + 1, 1 << 25, (1 << 25) + 1, 1 << 31)] == [8, 8, 8, 7, 1, 1, 1]
    assert [D.target(n) for n in (1, 2048 * 3500, 2048 * 3500 + 1)] == [2048, 2048, 2049]
    assert D.nbcap(16391) == 10 and D.nbcap(5_000_000) == 2443
    assert D.second_fine_level(8192, 4096, 32) and not D.second_fine_level(8192, 4096, 33) and not D.second_fine_level(4096, 4096, 5)


def test_the_cases_reach_what_the_docstring_says():
    """the cases of tests/_wx_worker.py by the model alone (what the runs add -- the tests left after a level -- is in
    tests/test_gpu_wilcoxon.py)"""
    import _wx_worker as W
    for name, (N, M, P, A, kind, seed, noise) in W.CASES.items():
        nv = N - N // 2
        want = "sorted" if name in W.CASES_SORTED else "cascade"
        assert D.path(nv, P, A) == want, name
    for name in W.CASES_CASCADE:
        N, M, P, A = W.CASES[name][:4]
        assert 16384 <= N - N // 2 <= 16391
        assert D.batches(N - N // 2, A, P * (A - 1), D.WX_NC0, 0, D.bc_bytes(N - N // 2, P * (A - 1)))[0]["R"] == 1
    # forced (every test open), the fine level of the many-tests cases: 2048 bins, two rows per thread from 88 tests (not at
    # 113 .. 116 and 145, where 1024 bins cost less), four from 177
    nv = 65537
    r_of = lambda A, n: D.batches(nv, A, n, D.pick_bins(n, nv), 1, D.bc_bytes(nv, n))[0]["R"]
    assert [r_of(8, n) for n in (87, 88, 112, 113, 117, 176, 177, 224)] == [1, 2, 2, 1, 2, 2, 4, 4]
    assert [r_of(16, n) for n in (87, 88, 120)] == [1, 2, 2]
    assert {D.scores_kc(W.CASES[n][3]) for n in W.CASES_SORTED} == {2, 4, 8, 16, 32, "wide"}
