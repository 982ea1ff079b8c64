"""CPU checks of tests/_gram_dispatch.py, the tests' copy of the statistics pass's plan (gram_plan.h: abc_gram_plan_of; gram.hip: the
kernel tables behind launch_stats_accumulate): it gives what the plan function itself gives on every case of
tests/cxx/gram_plan_probe.cpp, the instantiations it can reach are exactly the entries of the kernel tables and nothing is launched
past them, so the copy and the source cannot drift apart unseen, the plan's numbers are pinned, and tests/test_gpu_stats.py's
cases reach what they claim to."""
import os
import re
import subprocess

from _gram_dispatch import FIELDS, GRAM_AUTO, GRAM_FP64, GRAM_I8, blocks, kernel_for, plan, reachable, shapes, work_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family -> (its kernel table in gram.hip, the kernel the table holds)
TABLES = {"vgpr": ("GRAM_VGPR_K", "k_gram"), "dma8": ("GRAM_DMA8_K", "k_gram_dma8"), "wide": ("GRAM_WIDE_K", "k_gram_wide"),
          "i8": ("GRAM_I8_K", "k_gram_i8")}


def _source():
    return open(os.path.join(ROOT, "abcsmc_amd", "csrc", "gram.hip")).read()


def _table(name, kernel):
    """the (C, CY) of the entries of one of the static const kernel tables; every entry sits in the slot [C][CY] it names"""
    text = re.search(r"static const \w+ %s\[11\]\[3\] = \{(.*?)\n\};" % name, _source(), re.S).group(1)
    rows = re.findall(r"\{([^{}]*)\}", text)
    assert len(rows) <= 11 and not re.sub(r"\{[^{}]*\}", "", text).strip(" ,\n"), text
    entry = r"nullptr|\b(k_\w+)<(\d+), (\d+)>"
    out = set()
    for C, row in enumerate(rows):
        entries = re.findall(entry, row)
        assert len(entries) <= 3 and not re.sub(entry, "", row).strip(" ,"), row
        for CY, (k, c, cy) in enumerate(entries):
            if k:
                assert k == kernel and (int(c), int(cy)) == (C, CY), (name, row)
                out.add((C, CY))
    return out


def _gram_table():
    """every (family, C, CY) instance the tables of the single-launch families hold"""
    return {(fam, C, CY) for fam, (name, kernel) in TABLES.items() for C, CY in _table(name, kernel)}


def _host_code():
    """gram.hip behind its kernel tables, without comments"""
    src = _source()
    return re.sub(r"//[^\n]*", "", src[src.index("template <typename F>\nstatic F gram_slot("):])


def test_mirror_reaches_exactly_the_kernel_tables():
    table = _gram_table()
    assert len(table) == 46, sorted(table)
    assert [len(_table(*TABLES[f])) for f in ("vgpr", "dma8", "wide", "i8")] == [15, 8, 9, 14]
    mirror = reachable()
    assert mirror == table, ("in the mirror only: %s; in gram.hip only: %s" % (sorted(mirror - table), sorted(table - mirror)))
    # k_gram_far beside every k_gram_i8; the reduce of every instance, the grouped kernels' (6, 0) among them
    assert _table("GRAM_FAR_K", "k_gram_far") == _table("GRAM_I8_K", "k_gram_i8")
    assert _table("STATS_REDUCE_K", "k_stats_reduce") == {(C, CY) for _, C, CY in table} | {(6, 0)}
    assert len(_table("STATS_REDUCE_K", "k_stats_reduce")) == 27
    src = _source()
    assert "static const GramDmaFn GRAM_GROUPED_DMA_K = k_gram_dma<6, 0, 4, true, 3, true>;" in src
    assert "static const GramFn GRAM_GROUPED_VGPR_K = k_gram<6, 0, true>;" in src


def test_nothing_is_launched_past_the_tables():
    """launch_stats_accumulate, the launch bodies and the grouped path launch through the tables and the named helper kernels only"""
    code = _host_code()
    launched = re.findall(r"hipLaunchKernelGGL\((\w+),", code)
    assert len(launched) == code.count("LaunchKernelGGL"), "a launch this reader does not understand"
    pointers = {"with_vec", "dma", "limbs", "far", "reduce"}
    assert set(launched) == pointers | {"k_pilot_scale", "k_group_table", "k_group_scatter", "k_pilot_shift"}, launched
    # the only kernels named behind the tables are the helpers; every pointer comes out of a table or is one of the grouped path's two
    assert set(re.findall(r"\bk_\w+", code)) == {"k_pilot_scale", "k_group_table", "k_group_scatter", "k_pilot_shift"}
    assert set(re.findall(r"gram_slot\((\w+), pl\)", code)) == {"GRAM_VGPR_K", "GRAM_DMA8_K", "GRAM_WIDE_K", "GRAM_I8_K", "GRAM_FAR_K",
                                                                 "STATS_REDUCE_K"}
    for decl, sources in (("const GramFn with_vec = ", ("gram_slot(GRAM_VGPR_K, pl)", "gram_slot(GRAM_WIDE_K, pl)", "GRAM_GROUPED_VGPR_K")),
                          ("const GramDmaFn dma = ", ("gram_slot(GRAM_DMA8_K, pl)", "GRAM_GROUPED_DMA_K")),
                          ("const GramI8Fn limbs = ", ("gram_slot(GRAM_I8_K, pl)",)), ("const GramFarFn far = ", ("gram_slot(GRAM_FAR_K, pl)",)),
                          ("const StatsReduceFn reduce = ", ("gram_slot(STATS_REDUCE_K, pl)",))):
        for stmt in re.findall(re.escape(decl) + r"(.*?);", code, re.S):
            assert set(re.findall(r"gram_slot\(\w+, pl\)|GRAM_GROUPED_\w+_K", stmt)) == set(sources), stmt
        assert code.count(decl) >= 1
    assert code.count("StatsReduceFn reduce") == 3            # (two declarations and run_stats_reduce's parameter)
    # an empty slot is an error, not a fall-through
    assert code.count("return gram_no_instance(ctx, pl);") == 2 and "ABC_ERR_UNSUPPORTED" in code


def _probe_requests(M, P):
    """the requests tests/cxx/gram_plan_probe.cpp makes for one shape, in its order: (n, ldx, ldy, x_aligned, y_aligned, row0,
    n_train_global, n_set, mode)"""
    modes = (GRAM_AUTO, GRAM_FP64, GRAM_I8)
    for n in (5000, 5001):
        for ldx in (n + 2, n + 3):
            for ldy in (n + 4, n + 5):
                for al in range(4):
                    yield n, ldx, ldy, al & 1, al >> 1, 0, n // 2, 0, GRAM_AUTO
    for n, nt in ((0, 0), (1, 0), (1, 1), (2, 1), (3, 1), (4, 2), (199998, 99999), (200000, 100000), (200002, 100001), (799998, 399999),
                  (800000, 400000), (800000, 399999), (800000, 400001), (800000, 800000), (800000, 0), (800002, 400001),
                  (1999998, 999999), (2000000, 1000000), (2000000, 2000000), (3000000, 1500000)):
        for mode in modes:
            yield n, n, n, 1, 1, 0, nt, 0, mode
    for n, row0, nt, n_set in ((4094, 0, 500000, 1000000), (4096, 0, 500000, 1000000), (4096, 600000, 500000, 1000000),
                               (8192, 498000, 500000, 1000000), (4096, 0, 399999, 800000), (4096, 0, 100000, 200000),
                               (4096, 0, 99999, 199999)):
        for mode in modes:
            yield n, n_set + (n_set & 1), n_set + (n_set & 1), 1, 1, row0, nt, n_set, mode
    for n in (5000, 5001):
        for nt in (0, 1, n // 2, n):
            yield n, n + (n & 1), n + (n & 1), 1, 1, 0, nt, 0, GRAM_AUTO
        for nt in (500, 3000, 100000):
            yield n, 20000, 20000, 1, 1, 1000, nt, 20000, GRAM_AUTO
    for tr, cap, extra in ((128, 256, 1), (128, 384, 1), (64, 128, 1), (128, 128, 1), (32, 127, 2)):
        base = tr * (2 * cap - extra)
        for n in (base - tr, base - tr + 1, base - tr + 2, base, base + tr + 1, base + tr + 2):
            for mode in (GRAM_AUTO, GRAM_FP64):
                yield n, 1000000, 1000000, 1, 1, 0, 500000, 1000000, mode
    for n in (2, 64, 65, 128, 129, 130, 256, 257, 258, 384, 385):
        yield n, n + (n & 1), n + (n & 1), 1, 1, 0, n, 0, GRAM_AUTO


def test_mirror_agrees_with_the_plan_function(tmp_path):
    """abc_gram_plan_of itself (tests/cxx/gram_plan_probe.cpp prints it) against _gram_dispatch.plan on every case of the probe; and
    no plan names an empty slot of the kernel tables"""
    exe = str(tmp_path / "gram_plan_probe")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cxx", "gram_plan_probe.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    table = _gram_table()
    reduces = _table("STATS_REDUCE_K", "k_stats_reduce")
    lines = iter(out.stdout.splitlines())
    seen, clamped, count = set(), set(), 0
    for M, P in shapes():
        for n, ldx, ldy, xa, ya, row0, nt, n_set, mode in _probe_requests(M, P):
            req, _, res = next(lines).partition(" -> ")
            assert req == "%d %d %d %d %d %d %d %d %d %d %d" % (M, P, n, ldx, ldy, xa, ya, row0, nt, n_set, mode), req
            p = plan(M, P, n, nt, ldx, ldy, 0 if xa else 8, 0 if ya else 8, mode, n_set, row0)
            assert res == " ".join(str(int(p[f]) if f != "kernel" else p[f]) for f in FIELDS), (req, res, p)
            fam = p["kernel"]
            if fam.startswith("grouped"):
                assert (p["kC"], p["kCY"]) == (6, 0) and p["launches"] == p["pairs"] == p["groups"] * (p["groups"] - 1) // 2
            else:
                assert (fam, p["kC"], p["kCY"]) in table and (p["kC"], p["kCY"]) == (p["C"], p["CY"]) and p["launches"] == 1, req
            assert (p["kC"], p["kCY"]) in reduces and p["G"] >= 1
            seen.add((fam, p["C"], p["CY"]))
            clamped.add((fam, "one" if p["G"] == 1 else "cap" if p["G"] == p["cap"] else "between"))
            count += 1
    assert next(lines, None) is None
    assert {s for s in seen if not s[0].startswith("grouped")} == table
    assert {(f, C > 10) for f, C, _ in seen if f.startswith("grouped")} == {(f, w) for f in ("grouped_dma", "grouped_vgpr") for w in (False, True)}
    # both ends of every family's clamp (the byte-limb kernel takes no set small enough for one work-group)
    assert clamped == {(f, e) for f in ("vgpr", "dma8", "wide", "i8", "grouped_dma", "grouped_vgpr") for e in ("one", "cap", "between")} - {("i8", "one")}
    print("%d plan lines compared" % count)


def test_mirror_decisions_at_the_thresholds():
    # shapes the fp64 families take at small sizes, whatever the mode
    assert kernel_for(32, 16, 5000, 2500) == ("vgpr", 3, 1)
    assert kernel_for(40, 20, 5000, 2500) == ("dma8", 4, 1)
    assert kernel_for(40, 20, 5001, 2500) == ("vgpr", 4, 1)                  # odd n: no 16-byte row pairs
    assert kernel_for(40, 20, 5000, 2500, ldx=5001) == ("vgpr", 4, 1)       # odd leading dimension
    assert kernel_for(40, 20, 5000, 2500, y_align=8) == ("vgpr", 4, 1)      # base pointer off by 8 bytes
    assert kernel_for(90, 6, 5000, 2500) == ("vgpr", 6, 0)                  # (6, 0): the epilogue does not fit the DMA kernel
    assert kernel_for(128, 16, 5000, 2500) == ("wide", 9, 1)
    assert kernel_for(100, 8, 5000, 2500) == ("grouped_dma", 7, 0)
    assert kernel_for(100, 8, 5001, 2500) == ("grouped_vgpr", 7, 0)
    assert kernel_for(170, 10, 5000, 2500) == ("grouped_dma", 12, 1)
    # the byte-limb kernel: 200 000 rows of the set under GRAM_I8, 400 000 in every partition under GRAM_AUTO, never under FP64
    assert kernel_for(128, 16, 200000, 100000, mode=GRAM_I8) == ("i8", 9, 1)
    assert kernel_for(128, 16, 199998, 100000, mode=GRAM_I8) == ("wide", 9, 1)
    assert kernel_for(128, 16, 200001, 100000, mode=GRAM_I8) == ("wide", 9, 1)   # odd n
    assert kernel_for(128, 16, 800000, 400000) == ("i8", 9, 1)
    assert kernel_for(128, 16, 800000, 400001) == ("wide", 9, 1)
    assert kernel_for(128, 16, 800000, 800000) == ("i8", 9, 1)              # one empty partition: the other one counts
    assert kernel_for(128, 16, 800000, 400000, mode=GRAM_FP64) == ("wide", 9, 1)
    assert kernel_for(64, 32, 2000000, 1000000, mode=GRAM_I8) == ("i8", 6, 2)
    assert kernel_for(64, 32, 1999998, 1000000, mode=GRAM_I8) == ("dma8", 6, 2)
    # a shard: n rows of a set of n_set (the row rule looks at the set, the kernel's own needs at the shard)
    assert kernel_for(128, 16, 8192, 500000, n_set=1000000) == ("i8", 9, 1)
    assert kernel_for(128, 16, 4094, 500000, n_set=1000000) == ("wide", 9, 1)
    assert kernel_for(128, 16, 8192, 500000, n_set=1000000, mode=GRAM_AUTO) == kernel_for(128, 16, 8192, 500000, n_set=1000000)
    assert blocks(7, 30) == (3, 2) and blocks(16, 0) == (1, 0) and blocks(17, 15) == (2, 0)


def test_work_group_caps():
    assert work_groups("vgpr", 3, 66000, 66000) == (256, 256)
    assert work_groups("vgpr", 4, 100000, 100000) == (384, 384)
    assert work_groups("dma8", 4, 17000, 17000) == (128, 128)
    assert work_groups("grouped_vgpr", 7, 33001, 33001) == (128, 128)
    assert work_groups("vgpr", 3, 1, 0) == (1, 256)
    # the same through the plan; the grouped k_gram<6, 0, true> keeps 128 where k_gram<6, 0> on dense columns has 384
    assert [plan(90, 6, 100000, 100000)[f] for f in ("kernel", "G", "cap")] == ["vgpr", 384, 384]
    assert [plan(100, 8, 100001, 100001)[f] for f in ("kernel", "kC", "kCY", "G", "cap")] == ["grouped_vgpr", 6, 0, 128, 128]
    assert [plan(128, 16, 800000, 400000)[f] for f in ("kernel", "G", "cap", "nrec")] == ["i8", 127, 127, 128]


def test_plan_numbers():
    """dynamic LDS and the partial record of one instance per family, derived by hand from the kernels' layouts"""
    def p(M, P, n=5000, **kw):
        return plan(M, P, n, n // 2, **kw)
    v = p(32, 16)
    assert (v["kernel"], v["C"], v["CY"], v["lds"], v["psz"], v["threads"]) == ("vgpr", 3, 1, 49920, 1376, 512)
    g = p(100, 8, 5001)
    assert (g["kernel"], g["kC"], g["kCY"], g["lds"], g["psz"], g["threads"]) == ("grouped_vgpr", 6, 0, 99840, 5568, 256)
    assert (p(50, 10)["kernel"], p(50, 10)["kC"], p(50, 10)["kCY"], p(50, 10)["lds"]) == ("dma8", 4, 0, 98304)
    assert (p(64, 32)["kernel"], p(64, 32)["kC"], p(64, 32)["kCY"], p(64, 32)["lds"]) == ("dma8", 6, 2, 147456)
    # k_gram_dma<6, 0, 4, true, 3, true>: four rings of three 16-row chunks; its 21-block epilogue stages two waves at a time (halved)
    d = p(100, 8)
    assert (d["kernel"], d["kC"], d["kCY"], d["lds"], d["tile_rows"], d["threads"]) == ("grouped_dma", 6, 0, 147456, 64, 256)
    assert 4 * 21 * 256 * 8 > 160 * 1024 and 4 * 3 * 96 * 16 * 8 == 147456 > 2 * 21 * 256 * 8
    assert (p(128, 16)["kernel"], p(128, 16)["C"], p(128, 16)["CY"], p(128, 16)["lds"]) == ("wide", 9, 1, 76032)
    assert [p(M, P)["lds"] for M, P in ((147, 6), (140, 20), (121, 36))] == [84480] * 3
    i = plan(128, 16, 1000000, 500000)
    assert (i["kernel"], i["C"], i["CY"], i["lds"], i["nraw"]) == ("i8", 9, 1, 154512, 3)
    assert (i["tmax"], i["far_words"], i["escale_bytes"], i["far_mask_bytes"], i["far_sum_bytes"]) == (15627, 245, 640, 250032, 3928)
    # two raw tiles from 157 columns on
    nraw = [plan(128, cols - 128, 1000000, 500000)["nraw"] for cols in range(145, 161)]
    assert nraw == [3] * 12 + [2] * 4
    assert all(plan(128, cols - 128, 1000000, 500000)["lds"] <= 160 * 1024 for cols in range(113, 161))
    # the grouped path: 48-column groups, every pair of them
    assert [(p(M, P)["groups"], p(M, P)["pairs"], p(M, P)["launches"]) for M, P in ((100, 8), (170, 10), (190, 18))] == \
        [(3, 3, 3), (4, 6, 6), (5, 10, 10)]


def test_the_gpu_cases_reach_every_fp64_instantiation():
    """tests/test_gpu_stats.py's parametrisation covers the k_gram / k_gram_dma8 / k_gram_wide tables completely, and both branches of
    the grouped path at 7 and at more than 10 column blocks (the i8 family: tests/test_gpu_parity.py, I8_INSTANCES)"""
    from test_gpu_stats import INSTANCES
    for M, P, n, split, expect, ldx, ldy, xoff, yoff in INSTANCES:
        assert kernel_for(M, P, n, split, ldx, ldy, 8 * xoff, 8 * yoff) == expect, (M, P, n, expect)
    fp64 = {t for t in _gram_table() if t[0] != "i8"}
    reached = {e for e in (t[4] for t in INSTANCES) if e[0] in ("vgpr", "dma8", "wide")}
    assert reached == fp64, sorted(fp64 - reached)
    grouped = {(e[0], e[1] > 10) for e in (t[4] for t in INSTANCES) if e[0].startswith("grouped")}
    assert grouped == {("grouped_dma", False), ("grouped_vgpr", False), ("grouped_dma", True), ("grouped_vgpr", True)}
