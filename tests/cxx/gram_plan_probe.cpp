// Prints abc_gram_plan_of (abcsmc_amd/csrc/gram_plan.h), the plan behind launch_stats_accumulate, one line per case, for
// tests/test_gram_dispatch.py to hold the tests' copy (tests/_gram_dispatch.py) against.  A line is the request, "->", the plan:
//   M P n ldx ldy x_aligned y_aligned row0 n_train_global n_set mode -> kernel C CY vec_ok dma_ok split kC kCY tile_rows threads G cap
//       nrec nblk psz partial_bytes lds tmax nraw far_words escale_bytes far_mask_bytes far_sum_bytes groups pairs launches
// Shapes: the first and the last column count of every number of column blocks up to 13, with the metrics ending on either side
// of every block boundary (every (C, CY), sets without metrics among them).  Per shape: both parities of n, ldx and ldy x the four
// alignments; whole sets on both sides of 2 rows, of 200 000 and 2 000 000 rows in the set and of 400 000 in a partition, one of
// them empty, in the three modes; shards on both sides of 4096 rows; the split at 0, 1, n / 2 and n and with a first row behind,
// inside and in front of the training rows; n at both ends of every clamp of the work-groups.
// g++ -O2 -std=c++17 tests/cxx/gram_plan_probe.cpp
#include <cstdio>

#include "../../abcsmc_amd/csrc/gram_plan.h"

static const char* name(abc_gram_kernel k) {
    switch (k) {
        case GRAM_VGPR: return "vgpr";
        case GRAM_DMA8: return "dma8";
        case GRAM_WIDE: return "wide";
        case GRAM_I8: return "i8";
        case GRAM_GROUPED_DMA: return "grouped_dma";
        default: return "grouped_vgpr";
    }
}

static void line(const abc_gram_request& q) {
    const abc_gram_plan p = abc_gram_plan_of(q);
    printf("%zu %zu %zu %zu %zu %d %d %llu %llu %zu %d -> %s %d %d %d %d %lld %d %d %d %d %d %d %d %d %d %zu %zu %lld %d %zu %zu %zu %zu %d %d %d\n",
           q.M, q.P, q.n, q.ldx, q.ldy, (int)q.x_aligned, (int)q.y_aligned, (unsigned long long)q.row0, (unsigned long long)q.n_train_global,
           q.n_set, q.gram_mode, name(p.kernel), p.C, p.CY, (int)p.vec_ok, (int)p.dma_ok, p.split, p.kC, p.kCY, p.tile_rows, p.threads, p.G,
           p.cap, p.nrec, p.nblk, p.psz, p.partial_bytes, p.lds, p.tmax, p.nraw, p.far_words, p.escale_bytes, p.far_mask_bytes,
           p.far_sum_bytes, p.groups, p.pairs, p.launches);
}

static void shape(size_t M, size_t P) {
    static const int MODES[3] = {ABC_GRAM_AUTO, ABC_GRAM_FP64, ABC_GRAM_I8};
    // both parities of n, ldx and ldy, the four alignments
    for (size_t n = 5000; n <= 5001; n++)
        for (size_t ldx = n + 2; ldx <= n + 3; ldx++)
            for (size_t ldy = n + 4; ldy <= n + 5; ldy++)
                for (int al = 0; al < 4; al++) line({n, ldx, ldy, M, P, (al & 1) != 0, (al & 2) != 0, 0, n / 2, 0, ABC_GRAM_AUTO});
    // whole sets (n, training rows), contiguous
    static const size_t SETS[][2] = {{0, 0}, {1, 0}, {1, 1}, {2, 1}, {3, 1}, {4, 2}, {199998, 99999}, {200000, 100000}, {200002, 100001},
                                     {799998, 399999}, {800000, 400000}, {800000, 399999}, {800000, 400001}, {800000, 800000}, {800000, 0},
                                     {800002, 400001}, {1999998, 999999}, {2000000, 1000000}, {2000000, 2000000}, {3000000, 1500000}};
    for (const auto& s : SETS)
        for (int mode : MODES) line({s[0], s[0], s[0], M, P, true, true, 0, s[1], 0, mode});
    // shards (n, row0, training rows of the set, rows of the set): views into the whole set's columns
    static const size_t SHARDS[][4] = {{4094, 0, 500000, 1000000}, {4096, 0, 500000, 1000000}, {4096, 600000, 500000, 1000000},
                                       {8192, 498000, 500000, 1000000}, {4096, 0, 399999, 800000}, {4096, 0, 100000, 200000},
                                       {4096, 0, 99999, 199999}};
    for (const auto& s : SHARDS)
        for (int mode : MODES) line({s[0], s[3] + (s[3] & 1), s[3] + (s[3] & 1), M, P, true, true, s[1], s[2], s[3], mode});
    // the split
    for (size_t n = 5000; n <= 5001; n++) {
        const size_t NT[4] = {0, 1, n / 2, n};
        for (size_t nt : NT) line({n, n + (n & 1), n + (n & 1), M, P, true, true, 0, nt, 0, ABC_GRAM_AUTO});
        const size_t NTG[3] = {500, 3000, 100000};
        for (size_t nt : NTG) line({n, 20000, 20000, M, P, true, true, 1000, nt, 20000, ABC_GRAM_AUTO});
    }
    // the clamps of the work-groups, G = clamp((ceil(rows / tile) + extra) / 2, 1, cap): (tile, cap, extra) of every family; rows = n,
    // all of them training rows of a large set (so that the byte-limb kernel, which takes no small set, is among the cases)
    static const size_t CLAMPS[][3] = {{128, 256, 1}, {128, 384, 1}, {64, 128, 1}, {128, 128, 1}, {32, 127, 2}};
    for (const auto& c : CLAMPS) {
        const size_t base = c[0] * (2 * c[1] - c[2]);       // the last n of exactly 2 cap tiles
        const size_t NS[6] = {base - c[0], base - c[0] + 1, base - c[0] + 2, base, base + c[0] + 1, base + c[0] + 2};
        for (size_t n : NS) {
            line({n, 1000000, 1000000, M, P, true, true, 0, 500000, 1000000, ABC_GRAM_AUTO});
            line({n, 1000000, 1000000, M, P, true, true, 0, 500000, 1000000, ABC_GRAM_FP64});
        }
    }
    static const size_t FEW[] = {2, 64, 65, 128, 129, 130, 256, 257, 258, 384, 385};
    for (size_t n : FEW) line({n, n + (n & 1), n + (n & 1), M, P, true, true, 0, n, 0, ABC_GRAM_AUTO});
}

int main() {
    static char buf[1 << 20];
    setvbuf(stdout, buf, _IOFBF, sizeof(buf));
    for (size_t C = 1; C <= 13; C++)
        for (size_t cols = 16 * (C - 1) + 1; cols <= 16 * C; cols += 15)
            for (size_t mb = 0; mb <= C; mb++)          // the metrics end in block mb, on its first or on its last column (mb = 0: none)
                for (size_t M = mb ? 16 * (mb - 1) + 1 : 0; M <= 16 * mb && M <= cols; M += 15) shape(M, cols - M);
    return 0;
}
