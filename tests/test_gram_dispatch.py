"""CPU checks of tests/_gram_dispatch.py, the tests' copy of the statistics kernel choice (gram.hip: gram_kernel, gram_kernel_for):
the instantiations it can reach are exactly the GRAM_RUN lines of launch_stats_accumulate, so the copy and the table cannot drift
apart unseen, and tests/test_gpu_stats.py's cases reach what they claim to."""
import os
import re

from _gram_dispatch import GRAM_AUTO, GRAM_FP64, GRAM_I8, blocks, kernel_for, reachable, work_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gram_run_table():
    src = open(os.path.join(ROOT, "abcsmc_amd", "csrc", "gram.hip")).read()
    body = src[src.index("int launch_stats_accumulate("):]
    body = body[:body.index("#undef GRAM_RUN")]
    return {(f, int(c), int(cy)) for f, c, cy in re.findall(r"GRAM_RUN\((run_\w+),\s*(\d+),\s*(\d+)\)", body)}


def test_mirror_reaches_exactly_the_gram_run_table():
    table = _gram_run_table()
    assert len(table) == 46, sorted(table)
    mirror = reachable()
    assert mirror == table, ("in the mirror only: %s; in gram.hip only: %s" % (sorted(mirror - table), sorted(table - mirror)))


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


def test_the_gpu_cases_reach_every_fp64_instantiation():
    """tests/test_gpu_stats.py's parametrisation covers run_gram / run_gram_dma8 / run_gram_wide completely, and both branches of
    the grouped path at 7 and at more than 10 column blocks (the i8 family: tests/test_gpu_parity.py, I8_INSTANCES)"""
    from test_gpu_stats import INSTANCES
    run_of = {"vgpr": "run_gram", "dma8": "run_gram_dma8", "wide": "run_gram_wide"}
    for M, P, n, split, expect, ldx, ldy, xoff, yoff in INSTANCES:
        assert kernel_for(M, P, n, split, ldx, ldy, 8 * xoff, 8 * yoff) == expect, (M, P, n, expect)
    fp64 = {t for t in _gram_run_table() if t[0] != "run_gram_i8"}
    reached = {(run_of[e[0]], e[1], e[2]) for e in (t[4] for t in INSTANCES) if e[0] in run_of}
    assert reached == fp64, sorted(fp64 - reached)
    grouped = {(e[0], e[1] > 10) for e in (t[4] for t in INSTANCES) if e[0].startswith("grouped")}
    assert grouped == {("grouped_dma", False), ("grouped_vgpr", False), ("grouped_dma", True), ("grouped_vgpr", True)}
