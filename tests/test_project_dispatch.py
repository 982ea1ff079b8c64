"""CPU checks of tests/_project_dispatch.py, the tests' copy of the projection's kernel choice (project.hip:
launch_project_distance, launch_project_distance_scores): the kernels it can reach are exactly the launch sites of
launch_project_distance, so the copy and the source cannot drift apart unseen, and the decisions on both sides of every
threshold are pinned."""
import os
import re

from _project_dispatch import NOT_A_SHAPE, family, fused_plan, kc_of, mfma_lds, plan, reachable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch_table():
    """-> (main kernels, tail kernels) named at the launch sites of launch_project_distance"""
    src = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "project.hip")).read()
    body = src[src.index("int launch_project_distance("):]
    body = body[:body.index("size_t launch_project_scores(")]
    macro = lambda name: re.search(r"#define %s\(KCV\)(.*?)while \(0\)" % name, body, re.S).group(1)
    pd, pd_lds = macro("LAUNCH_PD"), macro("LAUNCH_PD_LDS")
    # what the two macros launch: the pair kernel, then the one-row kernel of the same width for the tail
    assert re.findall(r"k_project_\w+<KCV>", pd) == ["k_project_dist2<KCV>", "k_project_dist<KCV>"], pd
    assert re.findall(r"k_project_\w+<KCV>", pd_lds) == ["k_project_dist2_lds<KCV>", "k_project_dist<KCV>"], pd_lds
    calls, in_macro = [], False                                          # the launch sites, not the macro bodies
    for line in body.split("\n"):
        in_macro = in_macro or line.startswith("#define")
        if not in_macro:
            calls.append(line)
        in_macro = in_macro and line.rstrip().endswith("\\")
    calls = "\n".join(calls)
    mains, tails = set(), set()
    for kc in re.findall(r"LAUNCH_PD\((\d+)\)", calls):
        mains.add(("dist2", int(kc)))
        tails.add(("dist", int(kc)))
    for kc in re.findall(r"LAUNCH_PD_LDS\((\d+)\)", calls):
        mains.add(("dist2_lds", int(kc)))
        tails.add(("dist", int(kc)))
    for kt in re.findall(r"hipLaunchKernelGGL\(k_project_mfma<(\d+)>", calls):
        mains.add(("mfma", int(kt)))
    if re.search(r"hipLaunchKernelGGL\(k_project_dist_wide,", calls):
        mains.add(("wide",))
    if re.search(r"hipLaunchKernelGGL\(k_simple_dist,", calls):
        mains.add(("simple",))
    for kc in re.findall(r"hipLaunchKernelGGL\(k_project_dist<(\d+)>", calls):
        tails.add(("dist", int(kc)))
    # nothing else is launched from here
    named = set(re.findall(r"\b(k_[a-z0-9_]+)", calls))
    assert named == {"k_simple_dist", "k_pad_model", "k_project_dist_wide", "k_project_mfma", "k_project_dist"}, named
    return mains, tails


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
