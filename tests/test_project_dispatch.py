"""CPU checks of tests/_project_dispatch.py, the tests' copy of the projection's kernel choice (project_plan.h:
abc_project_plan; project.hip: the kernel tables behind launch_project_distance, launch_project_scores and
launch_project_distance_scores): it gives what the plan function itself gives on every case of
tests/cxx/project_plan_probe.cpp, the kernels it can reach are exactly the entries of the tables and the launch sites of
launch_project_distance, so the copy and the source cannot drift apart unseen, and the decisions on both sides of every
threshold are pinned."""
import functools
import os
import re
import subprocess

from _project_dispatch import NOT_A_SHAPE, STAGE, family, fused_plan, kc_of, mfma_lds, plan, reachable, scores_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    return open(os.path.join(ROOT, "abcsmc_amd", "csrc", "project.hip")).read()


def _table(name, kernel):
    """the widths of one of the static const kernel tables in the order of its entries (None: no entry)"""
    text = re.search(r"static const \w+ %s\[6\] = \{(.*?)\};" % name, _source(), re.S).group(1)
    entries = re.findall(r"nullptr|\b(k_\w+)<(\d+)>", text)
    assert all(k in ("", kernel) for k, _ in entries), entries
    return [int(w) if w else None for _, w in entries]


def _helper(name):
    """the text of a static helper of the three launchers"""
    src = _source()
    body = src[src.index("static %s(" % name):]
    return body[:body.index("\n}\n")]


def _launch_table():
    """-> (main kernels, tail kernels) launch_project_distance launches: by name, through the kernel tables, or through the
    two helpers that launch the kernels which also write scores"""
    src = _source()
    body = src[src.index("int launch_project_distance("):]
    body = body[:body.index("size_t launch_project_scores(")]
    # the tables are indexed by log2 of the width: the pair kernels, and the one-row kernel of the same width for the tail
    dist2, dist2_lds = _table("PROJECT_DIST2", "k_project_dist2"), _table("PROJECT_DIST2_LDS", "k_project_dist2_lds")
    dist = _table("PROJECT_DIST", "k_project_dist")
    for tab in (dist2, dist2_lds, dist):
        assert len(tab) == 6 and all(w in (None, 1 << i) for i, w in enumerate(tab)), tab
    assert "static int pj_lg(int KC) { return __builtin_ctz((unsigned)KC); }" in src
    assert len(re.findall(r"hipLaunchKernelGGL\(PROJECT_DIST2\[pj_lg\(KC\)\],", body)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(PROJECT_DIST\[pj_lg\(KC\)\],.*?X \+ pl\.rows, pl\.tail_rows,", body, re.S)) == 1
    pair_lds, mfma = _helper("void launch_pair_lds"), _helper("hipError_t launch_mfma")
    # the two helpers launch what they are given through pj_launch, with the caller's completion event or plainly
    assert re.findall(r"hip(?:Ext)?LaunchKernelGGL\((\w+)", _helper("void pj_launch")) == ["fn", "fn"]
    assert pair_lds.count("pj_launch(") == 1 and "pj_launch(PROJECT_DIST2_LDS[pj_lg(pl.KC)], pl, ctx->stream, done, " in pair_lds
    assert "LaunchKernelGGL" not in pair_lds and "LaunchKernelGGL" not in mfma
    assert "PROJECT_DIST2_LDS" not in body and len(re.findall(r"\blaunch_pair_lds\(", body)) == 1
    assert len(re.findall(r"\blaunch_mfma\(", body)) == 1
    mains, tails = set(), set()
    for kc in filter(None, dist2):
        mains.add(("dist2", kc))
    for kc in filter(None, dist2_lds):
        mains.add(("dist2_lds", kc))
    for kt in re.findall(r"pj_launch\(k_project_mfma<(\d+)>, pl, ctx->stream, done, ", mfma):
        mains.add(("mfma", int(kt)))
    assert mfma.count("pj_launch(") == 1
    if re.search(r"hipLaunchKernelGGL\(k_project_dist_wide,", body):
        mains.add(("wide",))
    if re.search(r"hipLaunchKernelGGL\(k_simple_dist,", body):
        mains.add(("simple",))
    for kc in filter(None, dist):
        tails.add(("dist", kc))
    # nothing else is launched from here: every launch is one by name or one through a table
    direct = re.findall(r"hipLaunchKernelGGL\((k_[a-z0-9_]+)", body)
    assert len(direct) + 2 == body.count("LaunchKernelGGL("), "a launch this reader does not understand"
    named = set(direct) | set(re.findall(r"\b(k_[a-z0-9_]+)", mfma))
    assert named == {"k_simple_dist", "k_pad_model", "k_project_dist_wide", "k_project_mfma"}, named
    assert set(re.findall(r"\b(k_[a-z0-9_]+)", body)) == {"k_simple_dist", "k_pad_model", "k_project_dist_wide"}
    return mains, tails


def _kernel(name, kc, lds_main):
    """a kernel as the probe prints it -> as the mirror names it"""
    if name == "none":
        return None
    if name == "simple":
        return ("simple",)
    if name == "mfma":
        assert kc == 32
        return ("mfma", 2, "stage" if lds_main == STAGE else "loadings")
    return (name, kc)


def test_mirror_agrees_with_the_plan_function(tmp_path):
    """abc_project_plan itself (tests/cxx/project_plan_probe.cpp prints it) against _project_dispatch.plan, scores_plan and
    fused_plan on every case of the probe, all three modes"""
    exe = str(tmp_path / "project_plan_probe")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cxx", "project_plan_probe.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    Ms = (1, 2, 20, 248, 249, 252, 511, 512, 560, 561, 1023, 1024, 1100)
    ns = (0, 1, 2, 3, 1000, 1001, 524288, 524290, 1048576, 1048577, 2097152, 2097154)
    seen = {"D": set(), "S": set(), "F": set()}

    @functools.lru_cache(maxsize=None)
    def score_result(res, M, A):
        """the answer of a score mode -> NOT_A_SHAPE or (kernel, rows); nothing is planned where it declines, and where it does
        not, the LDS and the grid are the distance mode's for the same kernel on these rows (a line repeats for many requests)"""
        declined, main, kc, rows, lds, lds_main, grid = res.split()
        if declined == "1":
            assert (main, rows, lds, lds_main, grid) == ("none", "0", "0", "0", "0"), res
            return NOT_A_SHAPE
        k = _kernel(main, int(kc), int(lds_main))
        d = plan(int(rows), 2, True, True, M, max(A, 5), False)
        assert (k, int(lds), int(grid)) == (d["main"], d["lds"], d["grid"]), res
        return k, int(rows)

    def distance_result(res):
        main, kc, rows, tail, tail_rows, pad, lds, lds_main, grid, tail_grid = res.split()
        kc, rows, tail_rows, lds_main, grid, tail_grid = int(kc), int(rows), int(tail_rows), int(lds_main), int(grid), int(tail_grid)
        k = _kernel(main, kc, lds_main)
        assert (tail == "none") == (tail_rows == 0) and (lds_main != 0) == (main == "mfma"), res
        # a second trip through the grid-stride loop: by row pairs in the pair kernels, never in the matrix-pipe kernel
        work = (tail_rows if k is None else 0 if k[0] == "mfma" else rows // 2 if k[0].startswith("dist2") else rows)
        return rows + tail_rows, {"main": k, "tail": _kernel(tail, kc, 0), "pad": pad == "1", "lds": int(lds), "grid": grid if k else tail_grid,
                                  "tail_grid": tail_grid, "second": work > 256 * (grid if k else tail_grid)}

    # the probe's cases in the probe's order (the requests are compared as text: two million lines)
    lines = iter(out.stdout.splitlines())
    for M in Ms:
        for A in range(98):
            for n in ns:
                fused = [("%d %d %d %d %d" % (al & 1, al >> 1 & 1, al >> 2, rt, sld), al == 7, rt, sld)
                         for al in range(8) for rt in (0, 1, n // 2, n) for sld in (n + 4, n + 5)]
                for ldx in (n + 2, n + 3):
                    head = "%d %d %d %d " % (M, A, n, ldx)
                    for xa, da in ((0, 0), (1, 0), (0, 1), (1, 1)):
                        req, _, res = next(lines).partition(" -> ")
                        assert req == "D %s%d %d" % (head, xa, da), req
                        rows, got = distance_result(res)
                        assert rows == n and got == plan(n, ldx, bool(xa), bool(da), M, A, A == 0), (req, res)
                        seen["D"].add(family(got["main"]))
                        req, _, res = next(lines).partition(" -> ")
                        assert req == "S %s%d %d" % (head, xa, da), req
                        got = score_result(res, M, A)
                        assert got == scores_plan(n, ldx, bool(xa and da), M, A), (req, res)
                        seen["S"].add(got if got is NOT_A_SHAPE else got[0])
                    fhead = "F " + head
                    for tail, aligned, rt, sld in fused:
                        req, _, res = next(lines).partition(" -> ")
                        assert req == fhead + tail, req
                        got = score_result(res, M, A)
                        want = fused_plan(n, ldx, aligned, M, A, rt, sld)
                        assert (got is NOT_A_SHAPE and want is NOT_A_SHAPE) or (got[0] == want and got[1] == n), (req, res)
                        seen["F"].add(want)
    assert next(lines, None) is None
    assert seen["D"] == _launch_table()[0] | {None}
    score_kernels = {("dist2_lds", 8), ("dist2_lds", 16), ("mfma", 2, "stage"), ("mfma", 2, "loadings"), NOT_A_SHAPE}
    assert seen["S"] == seen["F"] == score_kernels


def test_mirror_reaches_exactly_the_launch_sites():
    mains, tails = _launch_table()
    assert len(mains) == 11, sorted(mains)
    r_mains, r_tails, r_only = reachable()
    got = {family(k) for k in r_mains}
    assert got == mains, "in the mirror only: %s; in project.hip only: %s" % (sorted(got - mains), sorted(mains - got))
    assert r_tails == tails == r_only == {("dist", kc) for kc in (1, 2, 4, 8, 16, 32)}
    # in full: both layouts of the matrix-pipe kernel, the wide kernel on two, three and four chunks
    assert {k for k in r_mains if k[0] == "mfma"} == {("mfma", 2, "stage"), ("mfma", 2, "loadings")}
    assert {k for k in r_mains if k[0] == "wide"} == {("wide", 64), ("wide", 96), ("wide", 128)}


def _p(M, A, n=1000, ldx=None, xa=True, da=True, simple=False):
    return plan(n, n + (n & 1) if ldx is None else ldx, xa, da, M, A, simple)


def test_component_thresholds():
    assert [kc_of(A) for A in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97)] == \
        [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 96, 96, 128]
    assert _p(10, 1)["main"] == ("dist2", 1) and _p(10, 2)["main"] == ("dist2", 2) and _p(10, 3)["main"] == ("dist2", 4)
    assert _p(10, 4)["main"] == ("dist2", 4) and _p(10, 5)["main"] == ("dist2_lds", 8)
    assert _p(10, 8)["main"] == ("dist2_lds", 8) and _p(10, 9)["main"] == ("dist2_lds", 16)
    assert _p(10, 16)["main"] == ("dist2_lds", 16) and _p(10, 17)["main"] == ("mfma", 2, "stage")
    assert _p(10, 32)["main"] == ("mfma", 2, "stage") and _p(10, 33)["main"] == ("wide", 64)
    assert _p(10, 64)["main"] == ("wide", 64) and _p(10, 65)["main"] == ("wide", 96)
    # the tail of an odd row count has the width of the pair kernel; the wide and the simple kernel take every row themselves
    for A, kc in ((1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32)):
        assert _p(10, A, n=1001)["tail"] == ("dist", kc) and _p(10, A, n=1000)["tail"] is None
    assert _p(10, 33, n=1001)["tail"] is None and _p(10, 0, n=1001, simple=True) == {
        "main": ("simple",), "tail": None, "pad": False, "lds": 0, "grid": 4, "tail_grid": 0, "second": False}
    # k_pad_model: not for the LDS and the matrix-pipe kernel unless a tail needs the padded copy
    assert not _p(10, 8)["pad"] and _p(10, 8, n=1001)["pad"] and not _p(10, 20)["pad"] and _p(10, 20, n=1001)["pad"]
    assert _p(10, 4)["pad"] and _p(10, 40)["pad"] and _p(2000, 8)["pad"]


def test_lds_limits():
    # k_project_dist2_lds: the loadings and the observed scores in at most 64 KiB
    assert _p(511, 16) == {"main": ("dist2_lds", 16), "tail": None, "pad": False, "lds": 65536, "grid": 2, "tail_grid": 0,
                           "second": False}
    assert _p(512, 16)["main"] == ("dist2", 16) and _p(512, 16)["lds"] == 0 and _p(512, 16)["pad"]
    assert _p(1023, 8)["main"] == ("dist2_lds", 8) and _p(1023, 8)["lds"] == 65536
    assert _p(1024, 8)["main"] == ("dist2", 8) and _p(1024, 8)["lds"] == 0
    assert _p(511, 9)["lds"] == 65536 and _p(1023, 5)["lds"] == 65536          # (the padded width counts, not A)
    # k_project_mfma<2>: the score stage in front of the observed scores up to M4 = 248, the loadings from 252 on
    assert mfma_lds(248) == (8448, 67840, "stage") and mfma_lds(249) == (252 * 34, (252 * 34 + 32) * 8, "loadings")
    assert 248 * 34 == 8432 < 8448 < 252 * 34
    assert _p(248, 32)["main"] == ("mfma", 2, "stage") and _p(248, 32)["lds"] == 67840
    assert _p(249, 17)["main"] == ("mfma", 2, "loadings") and _p(249, 17)["lds"] == 68800
    assert _p(1, 17)["lds"] == 67840
    # ... up to 150 KiB: M = 560 is the last, then the scalar-operand row-pair kernel
    assert _p(560, 32)["main"] == ("mfma", 2, "loadings") and _p(560, 32)["lds"] == 152576 <= 150 * 1024
    assert mfma_lds(561)[1] == 153664 > 150 * 1024
    assert _p(561, 32) == {"main": ("dist2", 32), "tail": None, "pad": True, "lds": 0, "grid": 2, "tail_grid": 0, "second": False}
    assert _p(561, 17, n=1001)["tail"] == ("dist", 32)
    # 32 components never take the LDS row-pair kernel: where its loadings would fit, the matrix-pipe kernel has them
    assert all(_p(M, 32)["main"][0] == "mfma" for M in range(1, 561))


def test_vec_ok_conditions():
    for A, pair in ((3, ("dist2", 4)), (8, ("dist2_lds", 8)), (16, ("dist2_lds", 16)), (24, ("mfma", 2, "stage"))):
        kc = kc_of(A)
        assert plan(1000, 1000, True, True, 20, A, False)["main"] == pair
        off = {"main": None, "tail": ("dist", kc), "pad": True, "lds": 0, "grid": 4, "tail_grid": 4, "second": False}
        assert plan(1000, 1001, True, True, 20, A, False) == off            # an odd leading dimension
        assert plan(1000, 1000, False, True, 20, A, False) == off           # X 8 bytes off
        assert plan(1000, 1000, True, False, 20, A, False) == off           # dist 8 bytes off
        assert plan(1, 2, True, True, 20, A, False) == dict(off, grid=1, tail_grid=1)       # a single row
        assert plan(2, 2, True, True, 20, A, False)["main"] == pair and plan(3, 4, True, True, 20, A, False)["tail"] == ("dist", kc)
    # neither the wide nor the simple kernel asks
    assert plan(1000, 1001, False, False, 20, 40, False)["main"] == ("wide", 64)
    assert plan(1000, 1001, False, False, 20, 0, True)["main"] == ("simple",)
    assert plan(0, 0, True, True, 20, 8, False)["main"] is None and plan(0, 0, True, True, 20, 8, False)["tail"] is None


def test_grids_and_second_trips():
    # k_project_dist2<KC>: 4096 work-groups of 256 row pairs
    assert not plan(2097152, 2097152, True, True, 2, 2, False)["second"]
    p = plan(2097152 + 2, 2097152 + 2, True, True, 2, 2, False)
    assert p["second"] and p["grid"] == 4096 and p["main"] == ("dist2", 2)
    # k_project_dist2_lds: 1024
    assert not plan(524288, 524288, True, True, 4, 8, False)["second"]
    p = plan(524288 + 2, 524288 + 2, True, True, 4, 8, False)
    assert p["second"] and p["grid"] == 1024 and p["main"] == ("dist2_lds", 8)
    # one row per lane: 4096 work-groups of 256 rows
    for A, simple, xa, kern in ((3, False, False, None), (0, True, True, ("simple",)), (33, False, True, ("wide", 64))):
        assert not plan(1048576, 1048576, xa, True, 2, A, simple)["second"]
        p = plan(1048576 + 1, 1048576 + 2, xa, True, 2, A, simple)
        assert p["second"] and p["grid"] == 4096 and p["main"] == kern
    assert plan(1048576 + 1, 1048576 + 2, False, True, 2, 3, False)["tail"] == ("dist", 4)
    # the matrix-pipe kernel has no loop: one wave per 64 rows
    p = plan(3000001, 3000002, True, True, 20, 24, False)
    assert p["grid"] == (3000000 + 255) // 256 and not p["second"] and p["tail_grid"] == 1


def test_fused_plan():
    ok = dict(n=2000, ldx=2000, aligned=True, row_test=0, sld=2000)
    f = lambda M, A, **kw: fused_plan(M=M, A=A, **dict(ok, **kw))
    assert f(20, 8) == ("dist2_lds", 8) and f(20, 5) == ("dist2_lds", 8) and f(20, 12) == ("dist2_lds", 16)
    assert f(20, 24) == ("mfma", 2, "stage") and f(300, 17) == ("mfma", 2, "loadings")
    assert f(20, 4) == NOT_A_SHAPE and f(20, 33) == NOT_A_SHAPE                 # (no narrow and no wide kernel here)
    assert f(511, 16) == ("dist2_lds", 16) and f(512, 16) == NOT_A_SHAPE
    assert f(1023, 8) == ("dist2_lds", 8) and f(1024, 8) == NOT_A_SHAPE
    assert f(560, 24) == ("mfma", 2, "loadings") and f(561, 24) == NOT_A_SHAPE
    for kw in (dict(n=2001, ldx=2002, sld=2002), dict(ldx=2001), dict(aligned=False), dict(row_test=1), dict(sld=2001),
               dict(row_test=2000), dict(n=0)):
        assert f(20, 8, **kw) == NOT_A_SHAPE, kw
    assert f(20, 8, row_test=1000, sld=1000) == ("dist2_lds", 8)


def test_scores_plan():
    ok = dict(n=2000, ldx=2000, aligned=True)
    s = lambda M, A, **kw: scores_plan(M=M, A=A, **dict(ok, **kw))
    # up to 4 components run the 8-wide kernel (the fused pass declines them); more than 32 none
    assert s(20, 1) == s(20, 4) == s(20, 8) == (("dist2_lds", 8), 2000) and s(20, 9) == s(20, 16) == (("dist2_lds", 16), 2000)
    assert s(20, 17) == s(20, 32) == (("mfma", 2, "stage"), 2000) and s(300, 17) == (("mfma", 2, "loadings"), 2000)
    assert s(20, 33) == NOT_A_SHAPE and s(20, 0) == (("dist2_lds", 8), 2000)
    assert s(511, 16)[0] == ("dist2_lds", 16) and s(512, 16) == NOT_A_SHAPE
    assert s(1023, 3)[0] == ("dist2_lds", 8) and s(1024, 3) == NOT_A_SHAPE
    assert s(560, 24)[0] == ("mfma", 2, "loadings") and s(561, 24) == NOT_A_SHAPE
    # an odd n: the matrix-pipe kernel takes the even part, the row-pair kernel nothing
    assert s(20, 24, n=2001) == (("mfma", 2, "stage"), 2000) and s(20, 8, n=2001) == NOT_A_SHAPE and s(20, 24, n=3)[1] == 2
    for kw in (dict(ldx=2001), dict(aligned=False), dict(n=1), dict(n=0)):
        assert s(20, 8, **kw) == NOT_A_SHAPE and s(20, 24, **kw) == NOT_A_SHAPE, kw


def test_the_score_plans_cases_reach_every_outcome():
    """between them, the reductions of tests/_wx_worker.py that take the cascade (wx_scores: launch_project_scores on the
    validation rows, X + N // 2 with leading dimension N; X and S from allocations on 16-byte boundaries) and the fused cases of
    tests/test_gpu_project.py (launch_project_distance_scores, row_test = 0) reach every outcome of the two score plans"""
    import _wx_dispatch as WD
    import _wx_worker as W
    import test_gpu_project as TP
    reached = {}
    for name, (N, M, P, A, *_) in W.CASES.items():
        nv = N - N // 2
        if WD.path(nv, P, A) == "cascade":
            got = scores_plan(nv, N, (N // 2) % 2 == 0 and N % 2 == 0, M, A)
            reached.setdefault(got if got == NOT_A_SHAPE else got[0], []).append(name)
    assert reached[("dist2_lds", 8)] and reached[("mfma", 2, "stage")] and "c32_loadings" in reached[("mfma", 2, "loadings")]
    assert reached[NOT_A_SHAPE]                                     # (an odd first validation row: X + N // 2 is 8 bytes off)
    for N, M, A, nc, kern in TP.FUSED:
        assert fused_plan(N, N, True, M, A, 0, N) == kern
        reached.setdefault(kern, []).append((N, M, A))
    assert set(reached) == {("dist2_lds", 8), ("dist2_lds", 16), ("mfma", 2, "stage"), ("mfma", 2, "loadings"), NOT_A_SHAPE}, reached
