// The projection's plan (project.hip): everything launch_project_distance, launch_project_scores and launch_project_distance_scores
// derive from the shape of a call, computed in one place so that the three (and wilcoxon.hip / targets.hip, which round the component
// count the same way) cannot disagree.  Host-only, plain C++17 (no HIP headers): tests/cxx/project_plan_probe.cpp prints it and
// tests/test_project_dispatch.py holds the tests' copy of these decisions (tests/_project_dispatch.py) against it.
#pragma once
#include <stddef.h>

constexpr size_t PJ_LDS_PAIR = 64 * 1024;            // bytes of dynamic LDS k_project_dist2_lds may ask for
constexpr size_t PJ_LDS_MFMA = 150 * 1024;           // ... and k_project_mfma<2>
constexpr size_t PJ_MAX_BLOCKS = 256 * 16;           // work-groups of the grid-stride kernels
constexpr size_t PJ_MAX_BLOCKS_LDS = 1024;           // ... of k_project_dist2_lds (every work-group copies the loadings once)
constexpr size_t PJ_MFMA_STAGE = 4 * 64 * (32 + 1);  // doubles of k_project_mfma<2>'s score stage: four waves x 64 rows x (32 + 1)

// ncomp lives on the device; the kernels are compiled for the next power of two >= A (beyond 32: the next multiple of 32, taken in
// chunks of 32) and the unused components are zero-padded (exact, see k_pad_model)
inline int abc_project_kc(size_t A) {
    int KC = 1;
    while (KC < (int)A) KC *= 2;
    if (KC > 32) KC = (int)((A + 31) / 32) * 32;
    return KC;
}

// k_project_mfma<2>: the doubles in front of the observed scores and the bytes of dynamic LDS.  In front lies whichever is larger,
// the loadings, means and deviations (M4 x 34 doubles, M4 = M rounded up to four) or the epilogue's score stage, which overlays
// them: the loadings from M4 = 252 on (252 x 34 = 8568 > 8448 > 248 x 34)
struct abc_pj_mfma_lds { size_t main, bytes; };
inline abc_pj_mfma_lds abc_project_mfma_lds(size_t M) {
    const size_t M4 = (M + 3) & ~(size_t)3, load = M4 * 32 + 2 * M4, main = load > PJ_MFMA_STAGE ? load : PJ_MFMA_STAGE;
    return {main, (main + 32) * sizeof(double)};
}
// k_project_dist2_lds<KC>: the padded loadings and the observed scores
inline size_t abc_project_pair_lds(size_t M, int KC) { return (M * KC + KC) * sizeof(double); }

// distances of every row whatever the shape | the Wilcoxon rule's validation scores alone, of the rows it can take | both in one pass, or nothing
enum abc_pj_mode { PJ_DISTANCE, PJ_SCORES, PJ_FUSED };
// k_simple_dist | k_project_dist_wide (KC = 32 ceil(A / 32)) | k_project_mfma<2> | k_project_dist2_lds<KC> | k_project_dist2<KC> | k_project_dist<KC>
enum abc_pj_kernel { PJ_NONE, PJ_SIMPLE, PJ_WIDE, PJ_MFMA, PJ_DIST2_LDS, PJ_DIST2, PJ_DIST };

struct abc_pj_request {
    abc_pj_mode mode;
    size_t n, ldx, M, A;
    bool simple;                                // (distance mode)
    size_t row_test, sld;                       // (fused mode: the first row that is scored, the leading dimension of S)
    bool x_aligned, dist_aligned, s_aligned;    // X, dist, S on 16-byte boundaries (a pointer the mode does not take: true)
};
struct abc_pj_plan {
    bool declined;              // the score modes: not a shape for it, nothing is queued
    abc_pj_kernel main, tail;   // the kernel of the rows taken in pairs (or of all rows: simple, wide), PJ_NONE where pairs are not possible;
    size_t rows, tail_rows;     // PJ_DIST for the rows it leaves in distance mode (the odd last one, or all of them)
    int KC;                     // the padded component count of both
    bool pad;                   // k_pad_model runs: not for the LDS and the matrix-pipe kernel, which pad for themselves, unless a tail needs the copy
    size_t lds, lds_main;       // bytes of dynamic LDS of the main kernel; k_project_mfma<2>: the doubles in front of the observed scores
    unsigned grid, tail_grid;   // work-groups
};

inline unsigned abc_project_blocks(size_t rows, size_t cap) { return (unsigned)((rows + 255) / 256 > cap ? cap : (rows + 255) / 256); }

inline abc_pj_plan abc_project_plan(const abc_pj_request& rq) {
    abc_pj_plan pl = {};
    const size_t n = rq.n, M = rq.M;
    const bool dist_mode = rq.mode == PJ_DISTANCE;
    if (dist_mode && (n == 0 || rq.simple)) {
        if (n) { pl.main = PJ_SIMPLE; pl.rows = n; pl.grid = abc_project_blocks(n, PJ_MAX_BLOCKS); }
        return pl;
    }
    int KC = abc_project_kc(rq.A);
    if (rq.mode == PJ_SCORES && KC < 8) KC = 8;         // scores alone: up to 4 components run the 8-wide kernel (the fused pass declines them)
    pl.KC = KC;
    if (dist_mode && KC > 32) { pl.main = PJ_WIDE; pl.rows = n; pl.pad = true; pl.grid = abc_project_blocks(n, PJ_MAX_BLOCKS); return pl; }
    // row pairs with 16-byte loads and stores: an even leading dimension, everything the mode touches on 16-byte boundaries, two rows
    const size_t npairs = (rq.ldx % 2 == 0 && rq.x_aligned && rq.dist_aligned && rq.s_aligned) ? n / 2 : 0;
    const abc_pj_mfma_lds ml = abc_project_mfma_lds(M);
    // 17..32 components: the score contraction on the fp64 matrix pipe, with row pairs and while its LDS fits (16 components: the
    // vector kernel is 5-10 % faster, measured); 8 / 16: the loadings in LDS, up to 64 KiB of them
    const bool mfma = KC == 32 && npairs && ml.bytes <= PJ_LDS_MFMA;
    const bool lds = (KC == 8 || KC == 16) && npairs && abc_project_pair_lds(M, KC) <= PJ_LDS_PAIR;
    if (!dist_mode) {
        // the score modes have these two kernels only, and both store row pairs: into dist and S (fused: an even n, row_test and sld),
        // into columns of n rows (scores alone: an even n in the row-pair kernel; the matrix-pipe kernel leaves an odd last row to the caller)
        const bool odd = n & 1;
        pl.declined = !(mfma || lds) || (rq.mode == PJ_FUSED ? odd || (rq.row_test & 1) || (rq.sld & 1) || rq.row_test >= n : lds && odd);
        if (pl.declined) return pl;
    }
    pl.rows = 2 * npairs;
    pl.tail_rows = dist_mode ? n - pl.rows : 0;         // the odd last row (without row pairs: every row) through the one-row kernel of the same width
    if (pl.tail_rows) { pl.tail = PJ_DIST; pl.tail_grid = abc_project_blocks(pl.tail_rows, PJ_MAX_BLOCKS); }
    pl.pad = dist_mode && (pl.tail_rows || !(mfma || lds));
    if (mfma) {                                         // one wave per 64 rows, no loop
        pl.main = PJ_MFMA; pl.lds = ml.bytes; pl.lds_main = ml.main; pl.grid = (unsigned)((pl.rows + 255) / 256);
    } else if (lds) {
        pl.main = PJ_DIST2_LDS; pl.lds = abc_project_pair_lds(M, KC); pl.grid = abc_project_blocks(npairs, PJ_MAX_BLOCKS_LDS);
    } else if (npairs) {                                // scalar operands: up to 4 components, and whatever the two above do not take
        pl.main = PJ_DIST2; pl.grid = abc_project_blocks(npairs, PJ_MAX_BLOCKS);
    }
    return pl;
}
