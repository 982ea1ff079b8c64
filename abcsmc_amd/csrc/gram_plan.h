// The statistics pass's plan (gram.hip): everything launch_stats_accumulate derives from the shape of a call -- the column blocks, which
// kernel family and instance, rows per tile, work-groups and their cap, the partial records, the LDS, the byte-limb kernel's side
// arrays, the grouped path's pairs -- computed in one place, for the launchers and for a caller that arranges its streams around
// the byte-limb kernel (abc_gram_takes_i8).  Host-only, plain C++17 (no HIP headers): tests/cxx/gram_plan_probe.cpp prints it and
// tests/test_gram_dispatch.py holds the tests' copy of these decisions (tests/_gram_dispatch.py) against it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/abcsmc_hip.h"

// ---- the kernels' constants, as functions of the instance (C 16-column blocks of [X|Y], the trailing CY of them without a metric) ----
constexpr int GRAM_TR = 128;               // rows per tile of k_gram
constexpr int GRAM_TRP = GRAM_TR + 2;      // its LDS column stride in doubles (== 2 mod 32 -> conflict-free b64 reads)
constexpr int GRAM_TRW = 64;               // rows per tile of k_gram_wide (column stride GRAM_TRW + 2) and of k_gram_dma8
constexpr int GRAM_TRI = 32;               // rows per tile of k_gram_i8: one step of the i8 MFMA
constexpr size_t GRAM_LDS_MAX = 160 * 1024;
constexpr int gram_max(int a, int b) { return a > b ? a : b; }
constexpr int gram_blocks(size_t M, size_t P) { return (int)((M + P + 15) / 16); }
constexpr int gram_yblocks(size_t M, size_t P) {       // trailing blocks without any metric column: at most two are skipped
    return gram_blocks(M, P) - (int)((M + 15) / 16) > 2 ? 2 : gram_blocks(M, P) - (int)((M + 15) / 16);
}
constexpr int gram_nblk(int C, int CY) { return C * (C + 1) / 2 - CY * (CY + 1) / 2; }       // 16 x 16 Gram blocks: the pure-Y ones are skipped
constexpr int gram_psz(int C, int CY) { return gram_nblk(C, CY) * 256 + 2 * 16 * C; }        // doubles per work-group partial record
constexpr int gram_vgpr_nw(int C) { return C <= 3 ? 8 : 4; }                                  // waves per work-group of k_gram
// k_gram: the tile, or the partial record where that is larger
constexpr int gram_vgpr_lds_d(int C, int CY) { return gram_max(16 * C * GRAM_TRP, gram_psz(C, CY)); }
// the LDS-DMA kernels' epilogue stages four waves' accumulators (two where four records of NBLK x 256 doubles exceed the LDS)
constexpr int gram_epi_d(int C, int CY) {
    return (size_t)4 * gram_nblk(C, CY) * 256 * sizeof(double) <= GRAM_LDS_MAX ? 4 * gram_nblk(C, CY) * 256 : 2 * gram_nblk(C, CY) * 256;
}
// k_gram_dma, wave-private staging: NW rings of R chunks of 16 rows x 16 C columns | the epilogue | the column sums' park
constexpr int gram_dma_lds_d(int C, int CY, int NW, int R) {
    return gram_max(gram_max(NW * R * 16 * C * 16, gram_epi_d(C, CY)), C * 64 * NW);
}
// k_gram_dma8: eight rings of three chunks of 8 rows
constexpr int gram_dma8_lds_d(int C, int CY) { return gram_max(gram_max(8 * 3 * 16 * C * 8, gram_epi_d(C, CY)), C * 512); }
constexpr int gram_wide_lds_d(int C) { return 16 * C * (GRAM_TRW + 2); }
// k_gram_i8: two or three raw tiles (LDS-DMA targets: the real columns only, [column][16 row pairs]), TWO sets of byte planes, a 16-byte
// record per column (shift, high words of magic and limit), three sets of far flags (32 rows + any); the running column sums
// and sums of squares live in registers (a thread's (column, four rows) slots are the same in every tile) and pass through
// the raw tiles' space once, at the end
constexpr int gram_i8_c32(int C) { return 32 * ((C + 1) / 2); }                              // columns in 32-column super-blocks
constexpr int gram_i8_plane(int C) { return gram_i8_c32(C) * 32; }                           // bytes of a byte plane: 32 rows of every column
constexpr int gram_i8_fixed_b(int C) { return 8 * gram_i8_plane(C) + gram_i8_c32(C) * 16 + 3 * 48 + 256; }   // (+ 256 zero bytes: the "raw column" of the padding columns)
constexpr int gram_i8_raw_bytes(int cols) { return ((cols + 3) / 4) * 1024; }
constexpr int gram_i8_raw_tiles(int C, int cols) { return gram_i8_fixed_b(C) + 3 * gram_i8_raw_bytes(cols) <= (int)GRAM_LDS_MAX ? 3 : 2; }   // (two: 157..160 columns)
constexpr int gram_i8_lds_bytes(int C, int cols) { return gram_i8_fixed_b(C) + gram_i8_raw_tiles(C, cols) * gram_i8_raw_bytes(cols); }

// ---- which statistics kernel a set takes ------------------------------------------------------------------------------------------
// ONE decision, for launch_stats_accumulate and for a caller that arranges its streams around the byte-limb kernel (abc_gram_takes_i8).
// Up to 48 columns (C <= 3) the VGPR-staged k_gram is the default since its loads carry the non-temporal policy: 75 us against 84 us
// for the LDS-DMA kernel at N = 1e6, M = 32, P = 16 (0.68 against 0.60 of the HBM peak inside a generation); 49..96 columns run the
// eight-wave LDS-DMA variant (0.29 against 0.68 ms on the configs[3] shape).  LDS-DMA staging (dma_ok) needs 16-B aligned columns and
// an even row count (row pairs never straddle the array end).
// 4..6 column blocks (49..96 columns, e.g. BASELINE configs[3]: 64 metrics + 32 parameters): k_gram_dma8, EIGHT waves of
// wave-private staging in 8-row chunks (two waves per SIMD keep the fp64 matrix pipe busy: 0.36 -> 0.29 ms on the configs[3]
// shard against the four-wave, 16-row-chunk variant, which stays for the column-pointer-table mode of the grouped path).
// (6, 0) needs 172 KB for its epilogue and stays on the VGPR-staged kernel.
// 81..96 columns of a LARGE set (configs[3]: 64 metrics + 32 parameters, 1e7 rows) go through the byte-limb kernel of the wide
// sets (k_gram_i8): 1.59 ms against k_gram_dma8's 1.99 at 1e7 rows x 96 columns (0.60 against 0.48 of HBM: the fp64
// matrix pipe is 0.62 busy there), the same statistics to the byte products' error (section 4).  From 2e6 rows: where it was measured.
// WHERE THE BYTE-LIMB KERNEL IS THE DEFAULT (round 6).  Its noise -- every value rounded to a 32-bit grid -- is harmless at the
// Gram's own scale (4e-11 of sqrt(G_aa G_bb)) but not always at the LOADINGS: a component that fits noise works on cross
// products sqrt(rows) below that scale, with close eigenvalues, and tests/fuzz/wide_model_fuzz.py found a used loading column
// 4.3e-6 off the oracle's (fp64 kernels: 4e-10) at 66 000 training rows x 29 responses x 30 components -- BASELINE.json allows
// 1e-6.  The error falls faster than 1 / rows: 64 fuzzed sets whose partitions hold 450 000 rows and more stay within 2.6e-7
// (profiles/r06_wide_model_fuzz_big.json).  So ABC_GRAM_AUTO takes the kernel only where EVERY non-empty partition of the
// WHOLE set (training / validation rows: ntr_set, nte_set) has at least 400 000 rows -- configs[4] (5e5 + 5e5), configs[3]
// (5e6 + 5e6) -- and the fp64 kernels below that; ABC_GRAM_I8 is round 5's rule (200 000 rows in the whole set) for A/B runs and tests.
// 8..10 column blocks: one launch, the Gram blocks dealt out to the waves of a work-group -- large sets on the byte-limb kernel on the
// i8 matrix pipe (sums and the diagonal exact, off-diagonal products to ~1e-10 of sqrt(G_aa G_bb)); small ones, and all with
// ABC_GRAM_FP64 (A/B runs, tests), on the fp64 matrix pipe (k_gram_wide).  (LDS-DMA staging: 16-byte aligned columns, an even row
// count; from 200000 rows: the values are rounded to a 32-bit grid of 10 .. 19 sigma, noise of 3e-9 sigma per value that averages
// out with the square root of the rows -- 1e-10 of sqrt(G_aa G_bb) at 35000 rows per partition, which the 32nd loading of a
// 128-metric model amplifies to 2e-7; 4e-8 at 1e6 rows.)  7 blocks, 97..112 columns: the byte-limb kernel where it applies -- round
// 5; the fp64 one-launch kernel spills at that width, so small sets of it stay on the grouped path, which reads every column twice.
// (A rank whose shard the byte-limb kernel cannot take -- an odd row count, columns that are not 16-byte aligned, fewer than 4096
// rows -- runs the fp64 kernel on ITS rows: the rows' rule is the same on every rank, dma_ok and n are about what can run.)
// Wider sets, and the shapes without an instantiation ((1, 1), (2, 2): sets without metrics): column groups of 48, one launch per
// pair of groups (every column is read ceil(columns / 48) - 1 times) -- through the four-wave LDS-DMA kernel where dma_ok, through
// k_gram otherwise, both on a column-pointer table.
// k_gram<C, CY> | k_gram_dma8<C, CY> | k_gram_wide<C, CY> | k_pilot_scale, k_gram_i8<C, CY>, k_gram_far<C, CY> |
// per pair of groups: k_gram_dma<6, 0, 4, true, 3, true> | k_gram<6, 0, true>
enum abc_gram_kernel { GRAM_VGPR, GRAM_DMA8, GRAM_WIDE, GRAM_I8, GRAM_GROUPED_DMA, GRAM_GROUPED_VGPR };

struct abc_gram_request {
    size_t n, ldx, ldy, M, P;
    bool x_aligned, y_aligned;           // X, Y on 16-byte boundaries
    uint64_t row0, n_train_global;       // the first row's number in the whole set, the whole set's training rows: split = what of them lies in [row0, row0 + n)
    size_t n_set;                        // (0: n) the rows of the whole set these n are a shard of
    int gram_mode;                       // ABC_GRAM_AUTO / ABC_GRAM_FP64 / ABC_GRAM_I8
};
struct abc_gram_plan {
    abc_gram_kernel kernel;
    int C, CY;                           // the set's column blocks
    bool vec_ok, dma_ok;                 // 16-byte loads of row pairs (even leading dimensions, aligned bases) | and an even row count of at least 2
    long long split;                     // rows [0, split) are training rows, [split, n) validation rows
    // one launch of the Gram kernel and of k_stats_reduce behind it; the grouped kernels: of every pair of groups
    int kC, kCY;                         // the instance: (C, CY), the grouped kernels (6, 0) over a pair's 96 columns
    int tile_rows, threads;
    int G, cap;                          // work-groups per partition = clamp(tiles / 2, 1, cap): >= 2 tiles per work-group amortise its prologue / epilogue
    int nrec;                            // partial records per partition that k_stats_reduce reads: G, the byte-limb kernel G + 1 (k_gram_far's)
    int nblk, psz;                       // Gram blocks and doubles of a partial record
    size_t partial_bytes, lds;           // both partitions' records; bytes of dynamic LDS
    // the byte-limb kernel: 32-row tiles of a partition (t0 may start a row early), raw tiles in LDS, words of far_sum per partition
    long long tmax;
    int nraw;
    size_t far_words, escale_bytes, far_mask_bytes, far_sum_bytes;
    // the grouped kernels: 48-column groups, pairs of them = launches
    int groups, pairs;
    int launches;                        // of the Gram kernel (and of the reduce): 1, or pairs
};

inline abc_gram_plan abc_gram_plan_of(const abc_gram_request& rq) {
    abc_gram_plan pl = {};
    const size_t n = rq.n;
    const int C = pl.C = gram_blocks(rq.M, rq.P), CY = pl.CY = gram_yblocks(rq.M, rq.P);
    pl.vec_ok = rq.ldx % 2 == 0 && rq.ldy % 2 == 0 && rq.x_aligned && rq.y_aligned;
    pl.dma_ok = pl.vec_ok && n % 2 == 0 && n >= 2;
    const size_t rows_set = rq.n_set ? rq.n_set : n;
    const size_t ntr_set = rq.n_train_global < rows_set ? (size_t)rq.n_train_global : rows_set, nte_set = rows_set - ntr_set;
    const size_t part_min = (ntr_set && nte_set) ? (ntr_set < nte_set ? ntr_set : nte_set) : (ntr_set ? ntr_set : nte_set);
    const bool i8_rows = rq.gram_mode == ABC_GRAM_I8 ? rows_set >= 200000 : (rq.gram_mode == ABC_GRAM_AUTO && part_min >= 400000);
    const bool i8_ok = i8_rows && pl.dma_ok && n >= 4096;
    const abc_gram_kernel grouped = pl.dma_ok ? GRAM_GROUPED_DMA : GRAM_GROUPED_VGPR;
    if (C >= 7) pl.kernel = C > 10 ? grouped : i8_ok ? GRAM_I8 : C == 7 ? grouped : GRAM_WIDE;
    else if (C == 6 && CY >= 1 && i8_ok && rows_set >= 2000000) pl.kernel = GRAM_I8;
    else if (C >= 4 && pl.dma_ok && !(C == 6 && CY == 0)) pl.kernel = GRAM_DMA8;
    else pl.kernel = (C >= 3 || (C >= 1 && CY < C)) ? GRAM_VGPR : grouped;

    if (rq.n_train_global > rq.row0) pl.split = (long long)(rq.n_train_global - rq.row0 < n ? rq.n_train_global - rq.row0 : n);
    const bool is_grouped = pl.kernel == GRAM_GROUPED_DMA || pl.kernel == GRAM_GROUPED_VGPR;
    const int kC = pl.kC = is_grouped ? 6 : C, kCY = pl.kCY = is_grouped ? 0 : CY;
    int extra = 1;                       // tiles beyond the larger partition's rows / tile_rows: tiles start on an even row
    switch (pl.kernel) {
        case GRAM_VGPR:                  // resident work-groups: 2 x 8 waves or 3 x 4 waves per CU
            pl.tile_rows = GRAM_TR; pl.threads = 64 * gram_vgpr_nw(C); pl.cap = gram_vgpr_nw(C) == 8 ? 256 : 384;
            pl.lds = gram_vgpr_lds_d(C, CY) * sizeof(double);
            break;
        case GRAM_DMA8:                  // ~150 KB of LDS: one work-group (eight waves) per CU, 2 partitions x 128
            pl.tile_rows = GRAM_TRW; pl.threads = 512; pl.cap = 128;
            pl.lds = gram_dma8_lds_d(C, CY) * sizeof(double);
            break;
        case GRAM_WIDE:                  // 84 KB of LDS and 512 threads: one work-group per CU, 2 partitions x 128
            pl.tile_rows = GRAM_TRW; pl.threads = 512; pl.cap = 128;
            pl.lds = gram_wide_lds_d(C) * sizeof(double);
            break;
        case GRAM_I8:                    // 154 KB of LDS, 512 threads with ~250 registers: one work-group per CU; with k_gram_far's record
            //                              128 records per partition (k_stats_reduce splits them evenly over its 16 slices)
            pl.tile_rows = GRAM_TRI; pl.threads = 512; pl.cap = 127; extra = 2;
            pl.lds = (size_t)gram_i8_lds_bytes(C, (int)(rq.M + rq.P));
            break;
        case GRAM_GROUPED_DMA:           // four waves of 16-row chunks; 150 KB of LDS: one work-group per CU, 2 partitions x 128
            pl.tile_rows = 16 * 4; pl.threads = 256; pl.cap = 128;
            pl.lds = gram_dma_lds_d(6, 0, 4, 3) * sizeof(double);
            break;
        case GRAM_GROUPED_VGPR:          // 100 KB of LDS: one work-group per CU (128, not the 384 of k_gram<6, 0> on dense columns)
            pl.tile_rows = GRAM_TR; pl.threads = 64 * gram_vgpr_nw(6); pl.cap = 128;
            pl.lds = gram_vgpr_lds_d(6, 0) * sizeof(double);
            break;
    }
    const long long ntr = pl.split, nte = (long long)n - pl.split;
    const long long tiles = ((ntr > nte ? ntr : nte) + pl.tile_rows - 1) / pl.tile_rows + extra;
    pl.G = (int)(tiles / 2 < 1 ? 1 : tiles / 2 > pl.cap ? pl.cap : tiles / 2);
    pl.nrec = pl.G + (pl.kernel == GRAM_I8 ? 1 : 0);
    pl.nblk = gram_nblk(kC, kCY);
    pl.psz = gram_psz(kC, kCY);
    pl.partial_bytes = (size_t)2 * pl.nrec * pl.psz * sizeof(double);
    pl.launches = 1;
    if (pl.kernel == GRAM_I8) {
        pl.tmax = tiles;
        pl.nraw = gram_i8_raw_tiles(C, (int)(rq.M + rq.P));
        pl.far_words = (size_t)((tiles + 63) / 64);
        pl.escale_bytes = (size_t)gram_i8_c32(C) * sizeof(int);
        pl.far_mask_bytes = (size_t)2 * tiles * 8;
        pl.far_sum_bytes = (2 * pl.far_words + 1) * 8;                 // (the last word: any far row at all)
    }
    if (is_grouped) {
        pl.groups = (int)((rq.M + rq.P + 47) / 48);
        pl.launches = pl.pairs = pl.groups * (pl.groups - 1) / 2;
    }
    return pl;
}
