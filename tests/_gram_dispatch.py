"""What abc_stats_accumulate_dev runs: a copy of abc_gram_plan_of (abcsmc_amd/csrc/gram_plan.h), the one plan behind
launch_stats_accumulate in abcsmc_amd/csrc/gram.hip, so a test can state the kernel family and instantiation it means to reach and
check that it does.  tests/test_gram_dispatch.py holds this copy against the plan function itself, line by line over the cases
tests/cxx/gram_plan_probe.cpp prints, and against the kernel tables of gram.hip; tests/test_gpu_stats.py asserts every case's family
through it.

Families (abc_gram_kernel, and the kernel table the launch goes through):
    vgpr          GRAM_VGPR_K   k_gram<C, CY>: VGPR-staged tiles of 128 rows
    dma8          GRAM_DMA8_K   k_gram_dma8<C, CY>: LDS-DMA, eight waves, 64-row tiles (16-byte aligned columns, even n)
    wide          GRAM_WIDE_K   k_gram_wide<C, CY>: 8..10 column blocks in one launch, fp64
    i8            GRAM_I8_K     k_gram_i8<C, CY> (with GRAM_FAR_K: k_gram_far): byte limbs on the i8 matrix pipe (large sets)
    grouped_dma   pairs of 48-column groups through k_gram_dma<6, 0, 4, true, 3, true>
    grouped_vgpr  pairs of 48-column groups through k_gram<6, 0, true> (no LDS-DMA: odd n, ld or alignment)
"""
GRAM_AUTO, GRAM_FP64, GRAM_I8 = 0, 1, 2

TR, TRP = 128, 130              # rows per tile of k_gram, its LDS column stride in doubles
LDS_MAX = 160 * 1024

# the fields of a plan in the order tests/cxx/gram_plan_probe.cpp prints them
FIELDS = ("kernel", "C", "CY", "vec_ok", "dma_ok", "split", "kC", "kCY", "tile_rows", "threads", "G", "cap", "nrec", "nblk", "psz",
          "partial_bytes", "lds", "tmax", "nraw", "far_words", "escale_bytes", "far_mask_bytes", "far_sum_bytes", "groups", "pairs",
          "launches")


def blocks(M, P):
    """(C, CY): 16-column blocks of [X|Y], trailing blocks without a metric column (at most 2)"""
    C = (M + P + 15) // 16
    return C, min(C - (M + 15) // 16, 2)


def vec_ok(ldx, ldy, x_align=0, y_align=0):
    """x_align / y_align: the base pointers' addresses mod 16"""
    return ldx % 2 == 0 and ldy % 2 == 0 and x_align % 16 == 0 and y_align % 16 == 0


def dma_ok(n, ldx, ldy, x_align=0, y_align=0):
    return vec_ok(ldx, ldy, x_align, y_align) and n % 2 == 0 and n >= 2


def nblk(C, CY):
    return C * (C + 1) // 2 - CY * (CY + 1) // 2


def psz(C, CY):
    """doubles of a work-group's partial record"""
    return nblk(C, CY) * 256 + 2 * 16 * C


def _epilogue(C, CY):
    """the LDS-DMA kernels' epilogue: four waves' accumulators, two where four exceed the LDS"""
    four = 4 * nblk(C, CY) * 256
    return four if four * 8 <= LDS_MAX else four // 2


def _i8_fixed(C):
    c32 = 32 * ((C + 1) // 2)
    return 8 * c32 * 32 + c32 * 16 + 3 * 48 + 256


def i8_raw_tiles(C, cols):
    return 3 if _i8_fixed(C) + 3 * ((cols + 3) // 4) * 1024 <= LDS_MAX else 2


def _launch(fam, C, CY, cols):
    """(instance C, CY, rows per tile, extra tiles, work-group cap, threads, bytes of dynamic LDS) of a family's Gram launch"""
    if fam == "vgpr":
        nw = 8 if C <= 3 else 4
        return C, CY, TR, 1, 256 if nw == 8 else 384, 64 * nw, 8 * max(16 * C * TRP, psz(C, CY))
    if fam == "dma8":
        return C, CY, 64, 1, 128, 512, 8 * max(8 * 3 * 16 * C * 8, _epilogue(C, CY), C * 512)
    if fam == "wide":
        return C, CY, 64, 1, 128, 512, 8 * 16 * C * 66
    if fam == "i8":
        return C, CY, 32, 2, 127, 512, _i8_fixed(C) + i8_raw_tiles(C, cols) * ((cols + 3) // 4) * 1024
    if fam == "grouped_dma":        # four waves, rings of three 16-row chunks of 96 columns
        return 6, 0, 64, 1, 128, 256, 8 * max(4 * 3 * 96 * 16, _epilogue(6, 0), 6 * 256)
    assert fam == "grouped_vgpr", fam
    return 6, 0, TR, 1, 128, 256, 8 * max(96 * TRP, psz(6, 0))


def _family(C, CY, dma, n, ntr_set, nte_set, mode):
    rows_set = ntr_set + nte_set
    if ntr_set and nte_set:
        part_min = min(ntr_set, nte_set)
    else:
        part_min = ntr_set or nte_set
    i8_rows = rows_set >= 200000 if mode == GRAM_I8 else (mode == GRAM_AUTO and part_min >= 400000)
    i8_ok = i8_rows and dma and n >= 4096
    grouped = "grouped_dma" if dma else "grouped_vgpr"
    if C >= 7:
        return grouped if C > 10 else "i8" if i8_ok else grouped if C == 7 else "wide"
    if C == 6 and CY >= 1 and i8_ok and rows_set >= 2000000:
        return "i8"
    if C >= 4 and dma and not (C == 6 and CY == 0):
        return "dma8"
    return "vgpr" if (C >= 3 or (C >= 1 and CY < C)) else grouped


def _tiles(rows, tr, extra):
    return (rows + tr - 1) // tr + extra


def plan(M, P, n, n_train_global, ldx=None, ldy=None, x_align=0, y_align=0, mode=GRAM_AUTO, n_set=0, row0=0):
    """-> the whole plan of abc_stats_accumulate_dev for these arguments, a dict of FIELDS (ld None: contiguous, = n).  The grouped
    families have no (C, CY) instantiation of their own: C and CY are the set's, kC and kCY the launched (6, 0)."""
    ldx = n if ldx is None else ldx
    ldy = n if ldy is None else ldy
    C, CY = blocks(M, P)
    vec, dma = vec_ok(ldx, ldy, x_align, y_align), dma_ok(n, ldx, ldy, x_align, y_align)
    rows_set = n_set or n
    ntr_set = min(n_train_global, rows_set)
    fam = _family(C, CY, dma, n, ntr_set, rows_set - ntr_set, mode)
    split = min(n_train_global - row0, n) if n_train_global > row0 else 0
    kC, kCY, tr, extra, cap, threads, lds = _launch(fam, C, CY, M + P)
    tiles = _tiles(max(split, n - split), tr, extra)
    G = min(max(tiles // 2, 1), cap)
    i8, grouped = fam == "i8", fam.startswith("grouped")
    nrec = G + 1 if i8 else G
    far_words = (tiles + 63) // 64 if i8 else 0
    groups = (M + P + 47) // 48 if grouped else 0
    pairs = groups * (groups - 1) // 2
    return {"kernel": fam, "C": C, "CY": CY, "vec_ok": vec, "dma_ok": dma, "split": split, "kC": kC, "kCY": kCY, "tile_rows": tr,
            "threads": threads, "G": G, "cap": cap, "nrec": nrec, "nblk": nblk(kC, kCY), "psz": psz(kC, kCY),
            "partial_bytes": 2 * nrec * psz(kC, kCY) * 8, "lds": lds, "tmax": tiles if i8 else 0,
            "nraw": i8_raw_tiles(C, M + P) if i8 else 0, "far_words": far_words, "escale_bytes": 32 * ((C + 1) // 2) * 4 if i8 else 0,
            "far_mask_bytes": 2 * tiles * 8 if i8 else 0, "far_sum_bytes": (2 * far_words + 1) * 8 if i8 else 0, "groups": groups,
            "pairs": pairs, "launches": pairs if grouped else 1}


def kernel_for(M, P, n, n_train_global, ldx=None, ldy=None, x_align=0, y_align=0, mode=GRAM_AUTO, n_set=0):
    """-> (family, C, CY) that abc_stats_accumulate_dev runs for these arguments: the grouped path's family names the branch it
    takes, C and CY are the set's"""
    p = plan(M, P, n, n_train_global, ldx, ldy, x_align, y_align, mode, n_set)
    return p["kernel"], p["C"], p["CY"]


def work_groups(fam, C, n, split):
    """(work-groups per partition of the family's launch: the grid's x dimension, their cap)"""
    _, _, tr, extra, cap, _, _ = _launch(fam, C, 0, 16 * C)
    return min(max(_tiles(max(split, n - split), tr, extra) // 2, 1), cap), cap


def shapes(max_blocks=13):
    """(M, P) of every (C, CY) up to max_blocks column blocks, in the order of tests/cxx/gram_plan_probe.cpp: the first and the last
    column count of every block count, the metrics ending on the first or the last column of every block (or none at all)"""
    for C in range(1, max_blocks + 1):
        for cols in (16 * (C - 1) + 1, 16 * C):
            for mb in range(C + 1):
                for M in ((16 * (mb - 1) + 1, 16 * mb) if mb else (0,)):
                    if M <= cols:
                        yield M, cols - M


def reachable(max_blocks=13):
    """every (family, C, CY) of a single-launch family launch_stats_accumulate can reach, over shapes, alignments, row counts and
    modes"""
    out = set()
    for M, P in shapes(max_blocks):
        for x_align in (8, 0):
            for n, ntr in ((64, 32), (5000, 2500), (300000, 150000), (1000000, 500000), (3000000, 1500000), (3000000, 3000000)):
                for mode in (GRAM_AUTO, GRAM_FP64, GRAM_I8):
                    p = plan(M, P, n, ntr, x_align=x_align, mode=mode)
                    if not p["kernel"].startswith("grouped"):
                        out.add((p["kernel"], p["C"], p["CY"]))
    return out
