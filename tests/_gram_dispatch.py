"""Which statistics kernel abc_stats_accumulate_dev runs: a copy of gram_kernel() / gram_kernel_for() in
abcsmc_amd/csrc/gram.hip, so a test can state the kernel family and instantiation it means to reach and check that it does.
tests/test_gram_dispatch.py holds this copy against the GRAM_RUN table of gram.hip; tests/test_gpu_stats.py asserts every case's
family through it.

Families (the run_* function launch_stats_accumulate calls):
    vgpr          run_gram       k_gram<C, CY>: VGPR-staged tiles of 128 rows
    dma8          run_gram_dma8  k_gram_dma8<C, CY>: LDS-DMA, eight waves, 64-row tiles (16-byte aligned columns, even n)
    wide          run_gram_wide  k_gram_wide<C, CY>: 8..10 column blocks in one launch, fp64
    i8            run_gram_i8    k_gram_i8<C, CY>: byte limbs on the i8 matrix pipe (large sets)
    grouped_dma   run_gram_grouped, pairs of 48-column groups through k_gram_dma<6, 0, 4, true, 3, true>
    grouped_vgpr  run_gram_grouped, pairs of 48-column groups through k_gram<6, 0, true> (no LDS-DMA: odd n, ld or alignment)
"""
GRAM_AUTO, GRAM_FP64, GRAM_I8 = 0, 1, 2

RUN_OF = {"vgpr": "run_gram", "dma8": "run_gram_dma8", "wide": "run_gram_wide", "i8": "run_gram_i8"}


def blocks(M, P):
    """(C, CY): 16-column blocks of [X|Y], trailing blocks without a metric column (at most 2)"""
    C = (M + P + 15) // 16
    return C, min(C - (M + 15) // 16, 2)


def dma_ok(n, ldx, ldy, x_align=0, y_align=0):
    """x_align / y_align: the base pointers' addresses mod 16"""
    return ldx % 2 == 0 and ldy % 2 == 0 and n % 2 == 0 and x_align % 16 == 0 and y_align % 16 == 0 and n >= 2


def gram_kernel(C, CY, dma, n, ntr_set, nte_set, mode):
    rows_set = ntr_set + nte_set
    if ntr_set and nte_set:
        part_min = min(ntr_set, nte_set)
    else:
        part_min = ntr_set or nte_set
    i8_rows = rows_set >= 200000 if mode == GRAM_I8 else (mode == GRAM_AUTO and part_min >= 400000)
    i8_ok = i8_rows and dma and n >= 4096
    if C >= 7:
        return "grouped" if C > 10 else "i8" if i8_ok else "grouped" if C == 7 else "wide"
    if C == 6 and CY >= 1 and i8_ok and rows_set >= 2000000:
        return "i8"
    if C >= 4 and dma and not (C == 6 and CY == 0):
        return "dma8"
    return "vgpr" if (C >= 3 or (C >= 1 and CY < C)) else "grouped"


def kernel_for(M, P, n, n_train_global, ldx=None, ldy=None, x_align=0, y_align=0, mode=GRAM_AUTO, n_set=0):
    """-> (family, C, CY) that abc_stats_accumulate_dev runs for these arguments (ld None: contiguous, = n).  The grouped
    path has no (C, CY) instantiation of its own: its family names the branch it takes, C and CY are the set's."""
    ldx = n if ldx is None else ldx
    ldy = n if ldy is None else ldy
    C, CY = blocks(M, P)
    dma = dma_ok(n, ldx, ldy, x_align, y_align)
    rows_set = n_set or n
    ntr_set = min(n_train_global, rows_set)
    fam = gram_kernel(C, CY, dma, n, ntr_set, rows_set - ntr_set, mode)
    if fam == "grouped":
        fam = "grouped_dma" if dma else "grouped_vgpr"
    return fam, C, CY


# (rows per tile, extra tiles, work-group cap) of every family's launch (run_* in gram.hip; vgpr: in work_groups, the cap
# depends on the wave count): G = clamp(((rows of the larger partition + TR - 1) / TR + extra) / 2, 1, cap)
_GRID = {"dma8": (64, 1, 128), "wide": (64, 1, 128), "i8": (32, 2, 127), "grouped_dma": (64, 1, 128),
         "grouped_vgpr": (128, 1, 128)}


def work_groups(fam, C, n, split):
    """work-groups per partition of the kernel's launch (the grid's x dimension)"""
    if fam == "vgpr":
        tr, extra, cap = 128, 1, 256 if C <= 3 else 384
    else:
        tr, extra, cap = _GRID[fam]
    rows = max(split, n - split)
    return min(max(((rows + tr - 1) // tr + extra) // 2, 1), cap), cap


def reachable(max_cols=200):
    """every (run function, C, CY) launch_stats_accumulate can reach, over shapes, alignments, row counts and modes"""
    out = set()
    for M in range(1, max_cols + 1):
        for P in range(0, max_cols + 1 - M):
            C, CY = blocks(M, P)
            for dma in (False, True):
                for n, ntr, nte in ((64, 32, 32), (5000, 2500, 2500), (300000, 150000, 150000), (1000000, 500000, 500000),
                                    (3000000, 1500000, 1500000), (3000000, 3000000, 0)):
                    for mode in (GRAM_AUTO, GRAM_FP64, GRAM_I8):
                        fam = gram_kernel(C, CY, dma, n, ntr, nte, mode)
                        if fam != "grouped":
                            out.add((RUN_OF[fam], C, CY))
    return out
