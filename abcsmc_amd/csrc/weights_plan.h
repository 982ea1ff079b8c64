// The weight stage's plan (weights.hip): everything launch_weights_prev and launch_weights_raw derive from the shape of a call --
// padded width, chunks, which family of pair kernel, column slices, tiles, the far-row budget -- computed in one place, so the
// two launchers cannot disagree.  Host-only, plain C++17 (no HIP headers): tests/cxx/weights_plan_probe.cpp prints it and
// tests/test_weights_dispatch.py holds the tests' copy of these decisions (tests/_weights_dispatch.py) against it.
#pragma once
#include <stddef.h>

#include "../../include/abcsmc_hip.h"

constexpr int KS_NL = 4;                       // f16 operands per 16-parameter chunk and side
// The split kernel's variants, by their first template argument: 1, 2, 4 = 16-parameter chunks; KS_FOLD + 1, 2, 4 = as many chunks
// holding at most 13 / 29 / 61 parameters with the norm pieces in the three spare K-slots of the LAST chunk's limb operands -- hbTop (three f16 pieces against -1) in the
// exact h0.h0' step, hbLow (scaled by 2^24, three f16 pieces against -2^-24: f16 has no exponent for it otherwise) in the
// (h0 2^-11).(r2' 2^11) step, which only ever meets its own partner operand: 7 / 13 / 25 MFMAs per 1024 pairs instead of 9 / 15 / 27 (the -n
// step stays an instruction of its own: scripts/mfma_merge_probe.hip), and no norm operand to stream (the -1 entries the -n step
// needs are a per-lane constant).  The matrix pipe's energy is what bounds this kernel.
constexpr int KS_FOLD = 100;               // variant tag KS_FOLD + chunks: 101, 102, 104
// KS_TOPN + 1, 2, 4 = full chunks (14..16, 30..32, 62..64 parameters: no spare K-slot) with ONE MFMA less than the plain variants:
// the norm top is not subtracted by a step of its own in front of the batch reference but TOGETHER with the reference, in one
// bf16 step (-1 against the top pieces, the pieces of n against the -1 entries): X' - top - n is exact for every result within
// 2^-128 of the batch's largest (scripts/mfma_topn_probe.hip: 0 of 2 048 000 such results inexact), the others flush to zero
// anyway.  The reference has to come from X' = h0.h0' alone then: n = floor(max X' - tmin) with tmin the smallest top of the
// tile, which is only close to the largest X' - top if the tile's tops are close to one another -- so the previous set's tiles
// are filled in the ORDER OF THE ROWS' TOPS (launch_weights_prev: k_whb, a stable sort, k_wrows writing every row to its rank;
// pair sums do not care about the order of their terms): the spread inside a tile is the set's range / its tiles.  Taking the
// maximum of X' - top row by row instead (16 subtractions per lane and tile) cost more than the MFMA saved (+5.7 % at 16
// parameters); this way the vector pipe gets one subtraction per batch.
// The one-chunk kernel takes its batch over TWO consecutive tiles (weights.hip: kz_pair_sums): n = floor(max over both of max X' -
// tmin, each tile with its own tmin).  Every top of either tile is at least its tile's tmin, so X' - top - n <= 1 still holds for
// all 32 values, the largest of them is at least -KS_TOPN_SPREAD, and the partial sums of X' - top - n stay below 2^10 in units of
// 2^-14 for every result within 2^-126 of the largest of the 32 -- the operand ranges of the bf16 step are those of one tile
// (mfma_topn_probe); what lies further down flushes as before.  A tile whose tops spread over more than KS_TOPN_SPREAD (a "wide"
// tile of the sparse tail) has its top subtracted in a step of its own in front of the reference, from K-slots 8..10 where
// k_tile_tmin puts its pieces, so that the -top - n step -- the same instruction and operand for every tile -- finds slots 0..2 empty.
// The plan below does not know about any of this: a slice of an odd number of tiles ends with a one-tile batch inside the kernel.
constexpr int KS_TOPN = 200;

// 33..64 parameters: the previous tiles staged in LDS (k_kde_split_lds), and with it three stored chunks instead of four at 33..48
// parameters
inline int ks_chunks(size_t P) { return (P <= 16) ? 1 : (P <= 32) ? 2 : (P <= 48) ? 3 : 4; }
// up to 13 / 17..29 / 33..45 / 49..61 parameters: the variants of the split kernel with two MFMAs fewer (norm pieces in the spare K-slots: KS_FOLD)
inline bool ks_fold_on(size_t P, bool split) {
    return split && P + 3 <= (size_t)16 * ks_chunks(P);                       // three spare K-slots in the last chunk
}
// full chunks (no spare K-slot) and enough pairs for the sort to pay (it runs on the side stream of the fused drivers, in front of a
// stage-level call): the variants with one MFMA less.  minp: ABC_KDE_TOPN_MIN_PAIRS, read by the caller
inline bool ks_topn_on(bool split, bool fold, size_t pairs, double minp) {
    if (!split || fold) return false;
    return (double)pairs >= minp;
}

// column slices of the weight kernel (weights.hip) and the bytes of partial sums they need; shared with the
// workspace sizing in api.hip
inline size_t abc_kde_slices(size_t kn, size_t Kp, int PP) {
    if (kn == 0 || Kp == 0) return 1;
    size_t rows_per_slice = 24576 / (size_t)PP;            // ~190 KB of scaled previous-set rows per slice
    if (rows_per_slice < 256) rows_per_slice = 256;
    size_t s = (Kp + rows_per_slice - 1) / rows_per_slice;
    const size_t rb = (kn + 255) / 256;
    if (s * rb < 4096) s = (4096 + rb - 1) / rb;           // small sets: still a few work-groups per resident slot
    size_t cap = ((size_t)64 << 20) / (8 * kn);            // partial sums: slices x kn doubles <= 64 MB ...
    if (cap < 8) cap = 8;                                  // ... but at least 8 slices
    if (s > cap) s = cap;
    if (s > Kp / 64) s = Kp / 64;
    if (s < 1) s = 1;
    if (s > 1024) s = 1024;
    return s;
}

struct abc_wplan {
    int PP;                // padded width: the next power of two from 2 on, beyond 64 parameters the next multiple of 64
    int NCH;               // 16-parameter chunks (3: dealt out as four, three stored)
    bool epan, split, fold, topn;
    int V;                 // the split kernels' variant tag: NCH, KS_FOLD + NCH or KS_TOPN + NCH
    size_t rb, slices;     // the pair kernels' grid: 256-row blocks of the new set x column slices of the previous one
    size_t nbt, nat;       // 32-row tiles of the previous / the new set
    int opa, opb;          // 1 KiB operands per tile of the new / the previous set
    int lim_i;             // far new rows the fix-ups take: more, and the fp64 stand-in takes the call
};

// topn is the one field the two launchers settle differently: launch_weights_prev from the pair count, launch_weights_raw from
// what the prepared previous set holds
inline void abc_weights_plan_topn(abc_wplan* pl, bool topn) {
    pl->topn = topn;
    pl->V = pl->NCH + (pl->fold ? KS_FOLD : topn ? KS_TOPN : 0);
}

// kn: the rows of the call (launch_weights_prev: the most rows a call against this previous set will bring, kn_max)
inline abc_wplan abc_weights_plan(size_t P, size_t kn, size_t Kp, int kde_mode, int weight_kernel, double topn_min_pairs) {
    abc_wplan pl;
    pl.PP = 2;
    while (pl.PP < (int)P) pl.PP *= 2;
    if (P > 64) pl.PP = (int)((P + 63) / 64 * 64);
    pl.NCH = ks_chunks(P);
    pl.epan = weight_kernel == ABC_WEIGHT_EPANECHNIKOV;
    // split-operand kernel: 5 <= P <= 64 parameters (padded width 8, 16, 32 or 64: one, two or four 16-parameter chunks; below
    // that the fp64 body is as short), unless the caller asked for fp64
    pl.split = (pl.PP >= 8 && P <= 64 && kde_mode != ABC_KDE_FP64 && !pl.epan);
    pl.fold = ks_fold_on(P, pl.split);
    abc_weights_plan_topn(&pl, ks_topn_on(pl.split, pl.fold, Kp * kn, topn_min_pairs));
    pl.rb = (kn + 255) / 256;
    // Column slices: many short ones.  Work-groups are dispatched slice by slice, so the ~2000 resident groups all
    // stream the same few hundred KB of the previous set through the scalar cache / L2; with 6 slices of 2 MB each
    // (one residency) the same kernel was 25 % slower, waiting on scalar loads (measured: 6 -> 12.0 ms, 16 -> 10.0,
    // 64 -> 9.1, 128 -> 9.05 at K = K' = 1e5).  Bounded by the partial-sum buffer (slices x kn doubles <= 64 MB).
    pl.slices = abc_kde_slices(kn, Kp, pl.PP);
    if (pl.split) {
        // Every work-group of the split kernel loads its 32-64 KB of resident operands once per slice: with the 65 slices
        // the fp64 kernel likes that was 1.2 GB of fabric traffic per launch at K = K' = 1e5 (PMC).  Its time is flat between
        // 24 and 130 slices, so it gets about 12k work-groups (16 residencies of the chip) and no more.
        size_t cap = pl.rb ? 12288 / pl.rb : 12288;            // (rb = 0: a previous set prepared for no rows yet)
        if (cap < 8) cap = 8;
        if (pl.slices > cap) pl.slices = cap;
    }
    pl.nbt = (Kp + 31) / 32;
    pl.nat = pl.rb * 8;
    pl.opa = pl.NCH * KS_NL;
    pl.opb = pl.opa + (pl.fold ? 0 : 1);
    pl.lim_i = (int)(kn / 16 + 32);
    return pl;
}
