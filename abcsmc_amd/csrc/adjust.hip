// Local-linear regression adjustment of the batched ranking (abc_rank_targets_adjust_dev; the definition is in the header).
//
// The ranking (launch_rank_targets) leaves the scores of every row, S (N x A, column-major), and the targets' scores O in the
// arena.  Then, per batch of targets:
//   k_adj_table     (optional) one streaming pass: a row-major table [S(nc) | Y(P)] of all N rows, so that a retained row is one
//                   contiguous read instead of nc + P separate cache lines; taken when the retained rows outnumber N / 4
//   k_adj_moments   grid (row chunks, targets): the chunk's rows, shifted by the target's first retained row, staged in LDS; a
//                   thread owns groups of four entries of the (1 + nc) x (1 + nc + P) moment block [1 x'] w [1 x' theta'] and runs one
//                   sequential fma chain over the chunk's rows; the chunk's block goes to the workspace (no atomics)
//   k_adj_solve     one work-group per target: the chunks' blocks summed in chunk order, centred, the sweep in LDS (64 right-hand
//                   sides at a time), coef / rank / status
//   k_adj_apply     (only for theta / weight) the adjusted rows and the weights
// Under parameter transforms (abc_ctx_set_param_transf) the caller hands forward(Y) as Y, made once per call by k_tf_apply (N P
// logarithms, not B K P at every gather), so everything above runs on the transformed scale unchanged; k_adj_apply carries the
// adjusted rows back (tf_back_j, as sm_value of segment_dev.h does for the products).
// The tolerance path (abc_rank_targets_path_dev) ranks once at K_max and runs the regression at every tolerance K_t of a list:
//   k_adj_moments_path  k_adj_moments with one weight column and one set of accumulators per tolerance: the chunk's rows are staged
//                       once and the tolerances' chains run interleaved over the same LDS reads; tolerance t's chain stops at row K_t
//   k_adj_solve         grid (targets, tolerances): the blocks of the chunks below K_t
//   k_path_mean         the rejection mean of the first K_t rows and the bandwidth
// Under the heteroscedastic variance correction (abc_ctx_set_adjust_hcorr) a second fit follows every first one:
//   k_adj_moments2  grid (row chunks, targets): the chunk's rows staged raw, the parameter columns turned into z = 2 log|v - alpha|
//                   (v with aj_adjusted's bits) minus the first row's z, the scores shifted as in the first pass; the same ascending
//                   fma chains for the (1 + nc) x P block [1 x'] w z' only
//   k_adj_solve<true>  the first fit's C from the first pass's blocks (the same sums, so the same pivots), the new right-hand sides;
//                   hcoef, the skip rule and its counter
// and k_adj_apply<true> rescales the residual of every made value (aj_hcorr, as sm_value<.., true> of segment_dev.h).  All three are
// instances of their own: calls without the setting launch the code they launched before it existed.
// Under the ridge adjustment (abc_ctx_set_adjust_ridge) three kernels follow every k_adj_solve<false>, which still gives rank and
// status, and replace its coef:
//   k_adj_rsolve    grid (targets, penalties): the same sums and sweep with the diagonal of C penalised; alpha_l, beta_l and the
//                   swept left block M_l to the arena
//   k_adj_press     grid (row tiles, targets, penalties): the rows' leverages from M_l, the leave-one-out terms, one partial per
//                   (tile, penalty, parameter)
//   k_adj_pick      one work-group per target: PRESS per penalty, the pick, coef and the context's record
// Under row importance weights (abc_ctx_set_row_weights) a row's weight is k_e omega[i_e]: the kernels that make a weight
// (k_adj_moments, k_adj_moments_path, k_adj_moments2, k_adj_press, k_adj_apply) and k_path_mean have RW instances that read omega
// where the weight is made (aj_weight_rw), and k_adj_solve / k_adj_pick have RW instances for the all-zero rule (a slot whose
// weights sum to 0 is not swept).  Calls without the setting launch the RW = false instances, which never see omega.
// On the host one function queues a fit, aj_fit_chain: k_adj_moments, k_adj_solve, the ridge kernels, k_adj_moments2 and
// k_adj_solve<true> for a batch of targets at one K, in the chunks of aj_plan(K, ..).  The adjust call runs it once per batch.  The
// tolerance path, under the variance correction or ridge, calls it once per (batch, tolerance) with K = K_t behind its own
// solve, so slot (b, t) of hcoef, pick and press, and of coef under ridge, has the bits of the adjust call with K = K_t because
// it is that call's code with that call's arguments.  aj_call_setup is the set-up of both entries, and every arena block has one
// byte count (aj_*_bytes) that the allocation and abc_adjust_need / abc_path_need share.
// Chunk sizes depend on K only, tile sizes on (nc, P) only, and the gather paths copy the same bits: a target's outputs are the
// same alone and in any batch.
#include <math.h>

#include <vector>

#include "abc_internal.h"
#include "adjust_dev.h"

namespace {

constexpr int AJ_MAXA = 64;
constexpr int AJ_MAXP = 1024;
constexpr int AJ_RHS = 64;                                  // right-hand sides swept together by k_adj_solve
constexpr int AJ_TILE_DBL = 7680;                           // doubles of k_adj_moments' LDS (60 KiB)
constexpr int AJ_APPLY_DBL = 4096;                          // doubles of k_adj_apply's row tile (32 KiB) and of its LDS coefficients
constexpr size_t AJ_PART_BYTES = (size_t)256 << 20;         // moment blocks of one batch of targets
constexpr size_t AJ_TABLE_MAX_BYTES = (size_t)2 << 30;      // largest row-major table
constexpr unsigned AJ_MAX_GRID_Y = 65535;

// T[i W + c] = c < nc ? S[i + sld c] : Y[i + ldy (c - nc)]: 64 rows x 32 columns at a time through LDS
__global__ __launch_bounds__(256) void k_adj_table(const double* __restrict__ S, size_t sld, const double* __restrict__ Y, size_t ldy,
                                                   size_t N, int nc, int P, double* __restrict__ T) {
    __shared__ double tile[64][33];
    const int t = threadIdx.x, W = nc + P;
    for (size_t r0 = (size_t)blockIdx.x * 64; r0 < N; r0 += (size_t)gridDim.x * 64) {
        const int nr = (N - r0 < 64) ? (int)(N - r0) : 64;
        for (int c0 = 0; c0 < W; c0 += 32) {
            const int ncol = (W - c0 < 32) ? W - c0 : 32;
            for (int q = t; q < 64 * 32; q += 256) {                // lanes along rows: coalesced column reads
                const int r = q & 63, c = q >> 6;
                if (r < nr && c < ncol) {
                    const int cc = c0 + c;
                    tile[r][c] = (cc < nc) ? S[r0 + r + sld * (size_t)cc] : Y[r0 + r + ldy * (size_t)(cc - nc)];
                }
            }
            __syncthreads();
            for (int q = t; q < nr * ncol; q += 256) {
                const int r = q / ncol, c = q % ncol;
                T[(r0 + r) * (size_t)W + c0 + c] = tile[r][c];
            }
            __syncthreads();
        }
    }
}

// the moment-block row stride in LDS: room for four u-entries past every row-group start (padding columns hold 0)
__host__ __device__ __forceinline__ int aj_stride(int nc, int P) {
    const int D = 1 + nc + P, u4 = 4 * ((1 + nc + 3) / 4);
    return D > u4 ? D : u4;
}

// one entry group's chain over the staged rows: acc[u] += (w_r u_{g+u}(r)) v_c(r), r ascending; loads of four rows ahead of the
// four fmas of each (the rows' order within every acc[u] chain is kept)
__device__ __forceinline__ void aj_chain(const double* __restrict__ tv, const double* __restrict__ tw, int Ds, int nr, int c, int g,
                                         double acc[4]) {
    int r = 0;
    for (; r + 4 <= nr; r += 4) {
        double v[4], w[4], u[4][4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double* row = tv + (r + q) * Ds;
            v[q] = row[c];
            w[q] = tw[r + q];
#pragma unroll
            for (int k = 0; k < 4; k++) u[q][k] = row[g + k];
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] = fma(w[q] * u[q][k], v[q], acc[k]);
    }
    for (; r < nr; r++) {
        const double* row = tv + r * Ds;
        const double v = row[c], w = tw[r];
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] = fma(w * row[g + k], v, acc[k]);
    }
}

// nr rows of a tile, shifted by the target's first row: tv[r Ds + 0] = 1, [1 + c] = value c of row ix[r] minus shift[1 + c], 0 in the
// padding columns
__device__ __forceinline__ void aj_stage_rows(const AjSrc& src, const uint64_t* __restrict__ ix, const double* __restrict__ shift,
                                              double* __restrict__ tv, int nr, int nc, int P, int t) {
    const int D = 1 + nc + P, Wv = nc + P, Ds = aj_stride(nc, P);
    for (int q = t; q < nr * Wv; q += 256) {
        const int r = q / Wv, c = q % Wv;
        tv[r * Ds + 1 + c] = aj_val(src, (size_t)ix[r], c, nc) - shift[1 + c];
    }
    for (int r = t; r < nr; r += 256) {
        tv[r * Ds] = 1.0;
        for (int c = D; c < Ds; c++) tv[r * Ds + c] = 0.0;
    }
}

// the tolerances of a path, ascending (kernel argument)
constexpr int AJ_MAXT = 16;
struct AjKs {
    size_t K[AJ_MAXT];
};

// aj_chain for the tolerance lanes L0 .. TL - 1 at once, all of them over the same nr rows: every lane has its own weight column
// (tw + l TRp) and its own four sums, and runs the chain of aj_chain (the same operations in the same order); the lanes share the
// loads of u and v and their fmas are independent of one another
template <int TL, int L0>
__device__ __forceinline__ void aj_chain_lanes(const double* __restrict__ tv, const double* __restrict__ tw, int TRp, int Ds, int nr,
                                               int c, int g, double (&acc)[TL][4]) {
    constexpr int RU = 4;                                       // rows loaded ahead of their fmas, as aj_chain
    int r = 0;
    for (; r + RU <= nr; r += RU) {
        double v[RU], u[RU][4], w[TL][RU];
#pragma unroll
        for (int q = 0; q < RU; q++) {
            const double* row = tv + (r + q) * Ds;
            v[q] = row[c];
#pragma unroll
            for (int k = 0; k < 4; k++) u[q][k] = row[g + k];
#pragma unroll
            for (int l = L0; l < TL; l++) w[l][q] = tw[l * TRp + r + q];
        }
#pragma unroll
        for (int q = 0; q < RU; q++)
#pragma unroll
            for (int l = L0; l < TL; l++)
#pragma unroll
                for (int k = 0; k < 4; k++) acc[l][k] = fma(w[l][q] * u[q][k], v[q], acc[l][k]);
    }
    for (; r < nr; r++) {
        const double* row = tv + r * Ds;
        const double v = row[c];
#pragma unroll
        for (int l = L0; l < TL; l++) {
            const double w = tw[l * TRp + r];
#pragma unroll
            for (int k = 0; k < 4; k++) acc[l][k] = fma(w * row[g + k], v, acc[l][k]);
        }
    }
}
// l0: the first lane whose chain covers all nr rows of the tile (the tolerances ascend, so every later lane does too)
template <int TL, int L0 = 0>
__device__ __forceinline__ void aj_chain_from(int l0, const double* __restrict__ tv, const double* __restrict__ tw, int TRp, int Ds,
                                              int nr, int c, int g, double (&acc)[TL][4]) {
    if constexpr (L0 < TL) {
        if (l0 == L0) aj_chain_lanes<TL, L0>(tv, tw, TRp, Ds, nr, c, g, acc);
        else aj_chain_from<TL, L0 + 1>(l0, tv, tw, TRp, Ds, nr, c, g, acc);
    }
}

// k_adj_moments for the tolerances t0 .. t0 + TL - 1 of a path (t0 may be negative: the lanes below tolerance 0 are idle) over the
// ranking at K_max = ld; blocks of at most 256 entry groups only.  Grid (chunks of K_max, targets b0 + blockIdx.y).  The chunk's rows are staged once, up to the largest
// tolerance of the pass; lane l's chain runs over the rows e0 <= e < min(e1, K_l) with h = d_{K_l - 1} and its own fallback, and is
// absent (nothing written) when e0 >= K_l.  part[(((blockIdx.y T + t) nchs + chunk) U + r) D + c].
// RW: under row importance weights, w_e = k_e om[i_e] (aj_weight_rw; om is not read otherwise).
template <int TL, bool RW>
__global__ __launch_bounds__(256) void k_adj_moments_path(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist,
                                                          size_t ld, AjKs ks, int T, int t0, int nc, int P, int kernel, size_t CH,
                                                          int TR, size_t b0, size_t nchs, double* __restrict__ part,
                                                          const double* __restrict__ om) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x;
    const int U = 1 + nc, D = 1 + nc + P, Wv = nc + P, Ds = aj_stride(nc, P);
    const int Dp = (D + 1) & ~1, TRp = (TR + 1) & ~1;
    double* shift = sm;                  // [1 + c]: the first row's value c
    double* tw = sm + Dp;                // TL x TRp weights
    double* tv = tw + TL * TRp;          // TR x Ds
    const size_t b = b0 + blockIdx.y, chunk = blockIdx.x;
    const uint64_t* ix = idx + b * ld;
    const double* dd = dist + b * ld;
    const size_t e0 = chunk * CH;
    size_t Kl[TL], Kp = 0;
    double h[TL];
    bool rect[TL];
#pragma unroll
    for (int l = 0; l < TL; l++) {
        Kl[l] = (t0 + l >= 0 && t0 + l < T) ? ks.K[t0 + l] : 0;
        if (Kl[l] <= e0) Kl[l] = 0;                             // no part in this chunk (such lanes come first: ascending)
        if (Kl[l] > Kp) Kp = Kl[l];
        h[l] = Kl[l] ? dd[Kl[l] - 1] : 0.0;
        rect[l] = kernel == 1 || (Kl[l] && aj_fallback(dd, Kl[l]));
    }
    if (Kp == 0) return;                                        // (uniform)
    const size_t e1 = (e0 + CH < Kp) ? e0 + CH : Kp;
    const size_t i0 = (size_t)ix[0];
    for (int c = t; c < Wv; c += 256) shift[1 + c] = aj_val(src, i0, c, nc);
    const int J = D * ((U + 3) / 4);                            // <= 256
    const int c = t % D, g = 4 * (t / D);
    double acc[TL][4];
#pragma unroll
    for (int l = 0; l < TL; l++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[l][k] = 0.0;
    for (size_t r0 = e0; r0 < e1; r0 += (size_t)TR) {
        const int nr = (e1 - r0 < (size_t)TR) ? (int)(e1 - r0) : TR;
        int nrl[TL], l0 = 0;
#pragma unroll
        for (int l = 0; l < TL; l++) {
            nrl[l] = (Kl[l] <= r0) ? 0 : ((Kl[l] - r0 < (size_t)nr) ? (int)(Kl[l] - r0) : nr);
            if (nrl[l] < nr) l0 = l + 1;
        }
        __syncthreads();                                        // the shift is written, the previous tile consumed
        aj_stage_rows(src, ix + r0, shift, tv, nr, nc, P, t);
#pragma unroll
        for (int l = 0; l < TL; l++)
            for (int r = t; r < nrl[l]; r += 256)
                tw[l * TRp + r] = aj_weight_rw<RW>(dd[r0 + r], h[l], rect[l], om, RW ? (size_t)ix[r0 + r] : 0);
        __syncthreads();
        if (t >= J) continue;
#pragma unroll
        for (int l = 0; l < TL; l++)                            // a tolerance that ends inside the tile: its own shorter chain
            if (nrl[l] > 0 && nrl[l] < nr) aj_chain(tv, tw + l * TRp, Ds, nrl[l], c, g, acc[l]);
        aj_chain_from<TL>(l0, tv, tw, TRp, Ds, nr, c, g, acc);
    }
    if (t >= J) return;
#pragma unroll
    for (int l = 0; l < TL; l++) {
        if (!Kl[l]) continue;
        double* pp = part + (((size_t)blockIdx.y * T + t0 + l) * nchs + chunk) * (size_t)U * D;
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (g + u < U) pp[(size_t)(g + u) * D + c] = acc[l][u];
    }
}

// grid (targets, tolerances): post_mean[(b T + t) P + j] = the fp64 mean of Y[i_e, j] over e < K_t (NS = 256 / min(P, 256) threads
// per parameter, each the sum of every NS-th row in ascending order, then those sums in thread order: (K_t, P) only);
// hout[b T + t] = d_{K_t - 1}.  src is read for the parameters only (columns nc ..).
// RW (row importance weights): sum om_e Y_e / sum om_e instead, both sums in the order above (the numerator an fma chain, the
// weights' sum a second chain over the same rows, added up in the same thread order); 0 / 0 = NaN when every om_e is 0.
template <bool RW>
__global__ __launch_bounds__(256) void k_path_mean(AjSrc src, int nc, const uint64_t* __restrict__ idx, const double* __restrict__ dist,
                                                   size_t ld, AjKs ks, int T, int P, double* __restrict__ post_mean,
                                                   double* __restrict__ hout, const double* __restrict__ om) {
    __shared__ double red[RW ? 512 : 256];                          // RW: the weights' sums behind the numerators
    [[maybe_unused]] double* redw = red + 256;                                    // (RW instances only)
    const int t = threadIdx.x, tt = blockIdx.y;
    const size_t b = blockIdx.x, K = ks.K[tt];
    const uint64_t* ix = idx + b * ld;
    if (hout && t == 0) hout[b * T + tt] = dist[b * ld + K - 1];
    if (!post_mean || P == 0) return;
    const int PW = P < 256 ? P : 256, NS = 256 / PW;
    const int j = t % PW, s = t / PW;
    for (int j0 = 0; j0 < P; j0 += PW) {
        const bool mine = s < NS && j0 + j < P;
        double a = 0.0, sw = 0.0;
        if (mine) {
            if constexpr (RW) {
                for (size_t e = (size_t)s; e < K; e += (size_t)NS) {
                    const double w = om[(size_t)ix[e]];
                    a = fma(w, aj_val(src, (size_t)ix[e], nc + j0 + j, nc), a);
                    sw += w;
                }
            } else {
                for (size_t e = (size_t)s; e < K; e += (size_t)NS) a += aj_val(src, (size_t)ix[e], nc + j0 + j, nc);
            }
        }
        red[t] = a;
        if constexpr (RW) redw[t] = sw;
        __syncthreads();
        if (mine && s == 0) {
            for (int q = 1; q < NS; q++) a += red[q * PW + j];
            if constexpr (RW) {
                for (int q = 1; q < NS; q++) sw += redw[q * PW + j];
                post_mean[(b * T + tt) * (size_t)P + j0 + j] = a / sw;
            } else {
                post_mean[(b * T + tt) * (size_t)P + j0 + j] = a / (double)K;
            }
        }
        __syncthreads();
    }
}

// grid (chunks, targets b0 + blockIdx.y); part[((blockIdx.y pstride + chunk) U + r) D + c] = sum over the chunk's rows e (ascending) of
// (w_e u_r) v_c, u = [1, x'], v = [1, x', theta'], x' / theta' = the row's values minus those of the target's first row.  Rows are
// staged TR at a time.  A thread owns one group of four entries when the block has at most 256 groups and keeps their sums in
// registers; otherwise an entry's running sum passes between tiles through part.  The chain is the same either way and for every TR.
// ld: a target's rows start at idx + b ld (K itself, or K_max when the rows are a prefix of a longer ranking); pstride: blocks
// between two targets in part (the grid's chunk count, or more when other tolerances' blocks lie between).
// RW: under row importance weights, w_e = k_e om[i_e]: one more scattered 8-byte read per staged row, where the weight is made.
template <bool RW>
__global__ __launch_bounds__(256) void k_adj_moments(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist,
                                                     size_t ld, size_t K, int nc, int P, int kernel, size_t CH, int TR, size_t b0,
                                                     size_t pstride, double* __restrict__ part, const double* __restrict__ om) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x;
    const int U = 1 + nc, D = 1 + nc + P, Wv = nc + P, Ds = aj_stride(nc, P);
    const int Dp = (D + 1) & ~1, TRp = (TR + 1) & ~1;
    double* shift = sm;                  // [1 + c]: the first row's value c
    double* tw = sm + Dp;                // TR weights
    double* tv = tw + TRp;               // TR x Ds
    const size_t b = b0 + blockIdx.y, chunk = blockIdx.x;
    const uint64_t* ix = idx + b * ld;
    const double* dd = dist + b * ld;
    const size_t e0 = chunk * CH, e1 = (e0 + CH < K) ? e0 + CH : K;
    const double h = dd[K - 1];
    const bool rect = kernel == 1 || aj_fallback(dd, K);
    const size_t i0 = (size_t)ix[0];
    for (int c = t; c < Wv; c += 256) shift[1 + c] = aj_val(src, i0, c, nc);
    double* pp = part + ((size_t)blockIdx.y * pstride + chunk) * (size_t)U * D;
    const int nrg = (U + 3) / 4, J = D * nrg;
    const bool regs = J <= 256;
    double racc[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t r0 = e0; r0 < e1; r0 += (size_t)TR) {
        const int nr = (e1 - r0 < (size_t)TR) ? (int)(e1 - r0) : TR;
        __syncthreads();                                        // the shift is written, the previous tile consumed
        aj_stage_rows(src, ix + r0, shift, tv, nr, nc, P, t);
        for (int r = t; r < nr; r += 256) tw[r] = aj_weight_rw<RW>(dd[r0 + r], h, rect, om, RW ? (size_t)ix[r0 + r] : 0);
        __syncthreads();
        if (regs) {
            if (t < J) aj_chain(tv, tw, Ds, nr, t % D, 4 * (t / D), racc);
            continue;
        }
        for (int j = t; j < J; j += 256) {
            const int c = j % D, g = 4 * (j / D);
            double acc[4];
#pragma unroll
            for (int u = 0; u < 4; u++) acc[u] = (r0 == e0 || g + u >= U) ? 0.0 : pp[(size_t)(g + u) * D + c];
            aj_chain(tv, tw, Ds, nr, c, g, acc);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (g + u < U) pp[(size_t)(g + u) * D + c] = acc[u];
        }
    }
    if (regs && t < J) {
        const int c = t % D, g = 4 * (t / D);
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (g + u < U) pp[(size_t)(g + u) * D + c] = racc[u];
    }
}

// the second stage's moments (the variance correction).  Grid and chunks as k_adj_moments; coefficient slot b T + tt.
// part2[((blockIdx.y pstride + chunk) U + r) P + j] = sum over the chunk's rows e (ascending) of (w_e u_r) z'_j, u = [1, x'] as in the
// first pass, z'_j = z_e[j] - z_0[j], z = 2 log|v_e[j] - alpha_j| with v_e[j] = aj_adjusted of the raw row (the bits k_adj_apply gives).
// A row with a zero or non-finite residual makes entry (0, j) non-finite for good (w u_0 = w >= 0: NaN from 0 x inf, or an
// infinity that no finite term removes), which is how k_adj_solve sees the skip rule.  cf_lds: the slot's (1 + nc) x P
// coefficients staged in LDS.  RW: w_e = k_e om[i_e], as the first pass.
template <bool RW>
__global__ __launch_bounds__(256) void k_adj_moments2(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist,
                                                      size_t ld, size_t K, int nc, int P, int A, int kernel, size_t CH, int TR, size_t b0,
                                                      size_t pstride, const double* __restrict__ O, int KCO,
                                                      const double* __restrict__ coef, int T, int tt, int cf_lds,
                                                      double* __restrict__ part2, const double* __restrict__ om) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x;
    const int U = 1 + nc, D = 1 + nc + P, Wv = nc + P, Ds = aj_stride(nc, P);
    const int Dp = (D + 1) & ~1, TRp = (TR + 1) & ~1;
    double* shift = sm;                  // [1 + k]: the first row's score k; [1 + nc + j]: the first row's z_j
    double* tw = sm + Dp;                // TR weights
    double* tv = tw + TRp;               // TR x Ds
    double* cf = tv + (size_t)TR * Ds;   // (1 + nc) x P coefficients (cf_lds)
    const size_t b = b0 + blockIdx.y, chunk = blockIdx.x;
    const uint64_t* ix = idx + b * ld;
    const double* dd = dist + b * ld;
    const size_t e0 = chunk * CH, e1 = (e0 + CH < K) ? e0 + CH : K;
    const double h = dd[K - 1];
    const bool rect = kernel == 1 || aj_fallback(dd, K);
    const size_t i0 = (size_t)ix[0];
    const double* cg = coef + (b * (size_t)T + (size_t)tt) * (size_t)(A + 1) * P;     // alpha_j at [j], beta_kj at [(1 + k) P + j]
    const double* ob = O + b * (size_t)KCO;
    if (cf_lds)
        for (int q = t; q < U * P; q += 256) cf[q] = cg[q];
    const double* cc = cf_lds ? cf : cg;
    for (int c = t; c < nc; c += 256) shift[1 + c] = aj_val(src, i0, c, nc);
    __syncthreads();
    for (int j = t; j < P; j += 256) {
        const double v0 = aj_adjusted(aj_val(src, i0, nc + j, nc), [&](int k) { return aj_val(src, i0, k, nc) - ob[k]; }, cc + P + j,
                                      (size_t)P, nc);
        shift[1 + nc + j] = aj_logres(v0, cc[j]);
    }
    double* pp = part2 + ((size_t)blockIdx.y * pstride + chunk) * (size_t)U * P;
    const int nrg = (U + 3) / 4, J = P * nrg;
    const bool regs = J <= 256;
    double racc[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t r0 = e0; r0 < e1; r0 += (size_t)TR) {
        const int nr = (e1 - r0 < (size_t)TR) ? (int)(e1 - r0) : TR;
        __syncthreads();                                        // the shift is written, the previous tile consumed
        for (int q = t; q < nr * Wv; q += 256) {                // the rows, raw
            const int r = q / Wv, c = q % Wv;
            tv[r * Ds + 1 + c] = aj_val(src, (size_t)ix[r0 + r], c, nc);
        }
        for (int r = t; r < nr; r += 256) {
            tv[r * Ds] = 1.0;
            for (int c = D; c < Ds; c++) tv[r * Ds + c] = 0.0;
            tw[r] = aj_weight_rw<RW>(dd[r0 + r], h, rect, om, RW ? (size_t)ix[r0 + r] : 0);
        }
        __syncthreads();
        for (int q = t; q < nr * P; q += 256) {                 // theta_e[j] -> z'_e[j] (its own slot; the scores are only read)
            const int r = q / P, j = q % P;
            double* row = tv + r * Ds;
            const double v = aj_adjusted(row[1 + nc + j], [&](int k) { return row[1 + k] - ob[k]; }, cc + P + j, (size_t)P, nc);
            row[1 + nc + j] = aj_logres(v, cc[j]) - shift[1 + nc + j];
        }
        __syncthreads();
        for (int q = t; q < nr * nc; q += 256) {                // x' as the first pass staged it
            const int r = q / nc, k = q % nc;
            tv[r * Ds + 1 + k] = tv[r * Ds + 1 + k] - shift[1 + k];
        }
        __syncthreads();
        if (regs) {
            if (t < J) aj_chain(tv, tw, Ds, nr, 1 + nc + t % P, 4 * (t / P), racc);
            continue;
        }
        for (int j = t; j < J; j += 256) {
            const int jj = j % P, g = 4 * (j / P);
            double acc[4];
#pragma unroll
            for (int u = 0; u < 4; u++) acc[u] = (r0 == e0 || g + u >= U) ? 0.0 : pp[(size_t)(g + u) * P + jj];
            aj_chain(tv, tw, Ds, nr, 1 + nc + jj, g, acc);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (g + u < U) pp[(size_t)(g + u) * P + jj] = acc[u];
        }
    }
    if (regs && t < J) {
        const int jj = t % P, g = 4 * (t / P);
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (g + u < U) pp[(size_t)(g + u) * P + jj] = racc[u];
    }
}

// the second fit's inputs and outputs of k_adj_solve<true>
struct AjHcSolve {
    const double* part2;            // k_adj_moments2's blocks, nchs slots per target and tolerance
    const double* coef;             // the first fit (read)
    double* hcoef;                  // the second fit (written), laid out as coef, at slot b hstride + hoff
    unsigned long long* skipped;    // (slot, parameter) pairs the skip rule took
    size_t hstride, hoff;           // 1, 0; a tolerance path (one tolerance per launch): T, t
};

// one work-group per (target b0 + blockIdx.x, tolerance t = blockIdx.y of T; the adjustment itself: T = 1, ks.K[0] = ld = K): the
// moments of the rows below K_t (the blocks of the chunks e0 < K_t, summed in chunk order; part holds nchs block slots per target and
// tolerance), centred; the sweep; coef, rank and status at slot b T + t.
// HC (the variance correction's second fit): C, the means and so every pivot decision from the same blocks by the same operations;
// the right-hand sides from hs.part2, shifted by the first row's z; hs.hcoef instead of coef (a = zbar - g' xbar in row 0); a
// parameter is skipped (NaN in row 0, zeros below) when K <= nc + 2 or its moment sum w z' is not finite; rank and status stay.
// RW (row importance weights): the blocks are k_adj_moments<true>'s and the same code reads them; a slot whose weights' sum is not
// positive (every w_e = 0) takes the all-zero rule instead of the sweep: coef rows 0 .. nc NaN, the rows above 0, rank 0, status
// bit 2 beside the bits of their own rules; HC: every parameter of the slot skipped and counted.
template <bool HC, bool RW>
__global__ __launch_bounds__(256) void k_adj_solve(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist,
                                                   size_t ld, AjKs ks, int T, size_t CH, int nc, int P, int A, int kernel,
                                                   const double* __restrict__ O, int KCO, const double* __restrict__ part, int nchs,
                                                   size_t b0, double* __restrict__ coef, int32_t* __restrict__ rank,
                                                   int32_t* __restrict__ status, AjHcSolve hs) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ unsigned s_skip;
    const int t = threadIdx.x;
    const int U = 1 + nc, D = 1 + nc + P, NB = nc + AJ_RHS, ncp = (nc + 1) & ~1;
    double* C0 = sm;                        // nc x nc: the centred moments
    double* Wk = C0 + ((nc * nc + 1) & ~1); // nc x NB: [C | c] being swept
    double* xs = Wk + nc * NB;              // sum w x'
    double* xm = xs + ncp;                  // mean of x'
    double* xb = xm + ncp;                  // mean of x (observation-centred)
    double* colk = xb + ncp;
    double* kept = colk + ncp;              // 1.0: pivot kept
    double* rowk = kept + ncp;              // NB
    double* ts = rowk + NB;                 // AJ_RHS: sum w theta'
    double* tm = ts + AJ_RHS;               // mean of theta (not shifted)
    double* sW = tm + AJ_RHS;               // [0] sum of the weights, [1] pivot of this step
    const size_t bl = blockIdx.x, b = b0 + bl, K = ks.K[blockIdx.y], slot = b * T + blockIdx.y;
    const int nch = (int)((K + CH - 1) / CH);
    const size_t blk = (size_t)U * D;
    const double* pb = part + (bl * T + blockIdx.y) * (size_t)nchs * blk;
    const size_t i0 = (size_t)idx[b * ld];
    const size_t blk2 = (size_t)U * P;
    const double* pb2 = HC ? hs.part2 + (bl * T + blockIdx.y) * (size_t)nchs * blk2 : nullptr;
    const double* c1 = HC ? hs.coef + slot * (size_t)(A + 1) * P : nullptr;
    if (HC && t == 0) s_skip = 0;
    for (int q = t; q < U; q += 256) {
        double s = 0.0;
        for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + q];
        if (q == 0) sW[0] = s; else xs[q - 1] = s;
    }
    __syncthreads();
    const double W = sW[0];
    if constexpr (RW) {
        if (!(W > 0.0)) {                                           // (uniform) the all-zero rule
            const double qnan = __longlong_as_double(0x7ff8000000000000ll);
            if constexpr (HC) {
                double* cz = hs.hcoef + (b * hs.hstride + hs.hoff) * (size_t)(A + 1) * P;
                for (int q = t; q < (A + 1) * P; q += 256) cz[q] = (q < P) ? qnan : 0.0;
                if (t == 0 && P > 0 && hs.skipped) atomicAdd(hs.skipped, (unsigned long long)P);
            } else {
                double* cz = coef + slot * (size_t)(A + 1) * P;
                for (int q = t; q < (A + 1) * P; q += 256) cz[q] = (q / P <= nc) ? qnan : 0.0;
                if (t == 0) {
                    if (rank) rank[slot] = 0;
                    if (status) status[slot] = 4 | (nc > 0 ? 1 : 0) | ((kernel == 0 && aj_fallback(dist + b * ld, K)) ? 2 : 0);
                }
            }
            return;
        }
    }
    for (int k = t; k < nc; k += 256) {
        xm[k] = xs[k] / W;
        xb[k] = xm[k] + (aj_val(src, i0, k, nc) - O[b * KCO + k]);
    }
    __syncthreads();
    for (int q = t; q < nc * nc; q += 256) {
        const int k = q / nc, l = q % nc, lo = k < l ? k : l, hi = k < l ? l : k;
        double s = 0.0;
        for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + (size_t)(1 + lo) * D + 1 + hi];
        C0[q] = fma(-xm[lo], xs[hi], s);
    }
    double* cb = HC ? hs.hcoef + (b * hs.hstride + hs.hoff) * (size_t)(A + 1) * P : coef + slot * (size_t)(A + 1) * P;
    for (int j0 = 0; j0 == 0 || j0 < P; j0 += AJ_RHS) {
        const int nb = (P - j0 < AJ_RHS) ? P - j0 : AJ_RHS, NW = nc + nb;
        __syncthreads();                                        // C0 written, the previous batch's coefficients read
        for (int jj = t; jj < nb; jj += 256) {
            double s = 0.0;
            if constexpr (HC) {
                const int j = j0 + jj;
                for (int ch = 0; ch < nch; ch++) s += pb2[ch * blk2 + j];
                const double* ob = O + b * (size_t)KCO;
                const double v0 = aj_adjusted(aj_val(src, i0, nc + j, nc), [&](int k) { return aj_val(src, i0, k, nc) - ob[k]; },
                                              c1 + P + j, (size_t)P, nc);
                ts[jj] = s;
                tm[jj] = aj_logres(v0, c1[j]) + s / W;
                continue;
            }
            for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + 1 + nc + j0 + jj];
            ts[jj] = s;
            tm[jj] = aj_val(src, i0, nc + j0 + jj, nc) + s / W;
        }
        for (int q = t; q < nc * nc; q += 256) Wk[(q / nc) * NB + q % nc] = C0[q];
        __syncthreads();
        for (int q = t; q < nc * nb; q += 256) {
            const int k = q / nb, jj = q % nb;
            double s = 0.0;
            if constexpr (HC) {
                for (int ch = 0; ch < nch; ch++) s += pb2[ch * blk2 + (size_t)(1 + k) * P + j0 + jj];
            } else {
                for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + (size_t)(1 + k) * D + 1 + nc + j0 + jj];
            }
            Wk[k * NB + nc + jj] = fma(-xm[k], ts[jj], s);
        }
        __syncthreads();
        for (int k = 0; k < nc; k++) {
            const double d = Wk[k * NB + k], c0 = C0[k * nc + k];
            const bool keep = (c0 > 0.0) && (d > 1e-10 * c0);
            if (t == 0) kept[k] = keep ? 1.0 : 0.0;
            if (!keep) continue;                                // (uniform)
            for (int q = t; q < NW; q += 256) rowk[q] = (q == k) ? 1.0 / d : Wk[k * NB + q] / d;
            for (int i = t; i < nc; i += 256) colk[i] = Wk[i * NB + k];
            __syncthreads();
            for (int q = t; q < nc * NW; q += 256) {
                const int i = q / NW, j = q % NW;
                double v;
                if (i == k) v = rowk[j];
                else if (j == k) v = -colk[i] / d;
                else v = fma(-colk[i], rowk[j], Wk[i * NB + j]);
                Wk[i * NB + j] = v;
            }
            __syncthreads();
        }
        __syncthreads();
        for (int jj = t; jj < nb; jj += 256) {
            const int j = j0 + jj;
            if constexpr (HC) {
                if (K <= (size_t)nc + 2 || !isfinite(ts[jj])) {     // the skip rule
                    cb[j] = __longlong_as_double(0x7ff8000000000000ll);
                    for (int k = 0; k < A; k++) cb[(size_t)(1 + k) * P + j] = 0.0;
                    atomicAdd(&s_skip, 1u);
                    continue;
                }
            }
            double a = tm[jj];
            for (int k = 0; k < nc; k++) {
                const double be = (kept[k] != 0.0) ? Wk[k * NB + nc + jj] : 0.0;
                a = fma(-be, xb[k], a);
                cb[(size_t)(1 + k) * P + j] = be;
            }
            for (int k = nc; k < A; k++) cb[(size_t)(1 + k) * P + j] = 0.0;
            cb[j] = a;
        }
    }
    if constexpr (HC) {
        __syncthreads();
        if (t == 0 && s_skip && hs.skipped) atomicAdd(hs.skipped, (unsigned long long)s_skip);
        return;
    }
    if (t == 0) {
        int r = 0;
        for (int k = 0; k < nc; k++) r += kept[k] != 0.0;
        if (rank) rank[slot] = r;
        if (status) status[slot] = (r < nc ? 1 : 0) | ((kernel == 0 && aj_fallback(dist + b * ld, K)) ? 2 : 0);
    }
}

// ---- ridge adjustment with the penalty chosen by leave-one-out PRESS (abc_ctx_set_adjust_ridge; the definition is in the header) ----
// the penalties of the setting, ascending (kernel argument)
struct AjLam {
    double v[ABC_RIDGE_MAXL];
};

// doubles of one (slot, penalty) fit in the arena: [0] W, [1 + k] xm_k (the weighted mean of the shifted scores), then the
// (1 + nc) x P coefficients laid out as coef (row 0 alpha_l, row 1 + k beta_l[k]), then M_l (nc x nc)
__host__ __device__ __forceinline__ size_t aj_rfit_dbl(int nc, int P) { return (size_t)1 + nc + (size_t)(1 + nc) * P + (size_t)nc * nc; }

// the penalised sweep: one work-group per (target b0 + blockIdx.x, penalty blockIdx.y).  k_adj_solve<false> with T = 1 over
// again (the same sums in the same order, so W, the means, C and c have its bits) except that the diagonal of C becomes
// fma(lambda, C_kk, C_kk) before the sweep, the skip rule reading that diagonal; lambda == 0 leaves every bit.  The swept left
// block is kept: M_l = the inverse over the kept pivots, rows and columns of skipped pivots 0.  rfit[(bl L + l) aj_rfit_dbl ..].
__global__ __launch_bounds__(256) void k_adj_rsolve(AjSrc src, const uint64_t* __restrict__ idx, size_t ld, size_t K, size_t CH, int nc, int P,
                                                    const double* __restrict__ O, int KCO, const double* __restrict__ part, int nchs,
                                                    size_t b0, AjLam lam, double* __restrict__ rfit) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x;
    const int U = 1 + nc, D = 1 + nc + P, NB = nc + AJ_RHS, ncp = (nc + 1) & ~1;
    double* C0 = sm;                        // nc x nc: the centred moments, the diagonal penalised
    double* Wk = C0 + ((nc * nc + 1) & ~1); // nc x NB: [C | c] being swept
    double* xs = Wk + nc * NB;
    double* xm = xs + ncp;
    double* xb = xm + ncp;
    double* colk = xb + ncp;
    double* kept = colk + ncp;
    double* rowk = kept + ncp;              // NB
    double* ts = rowk + NB;                 // AJ_RHS
    double* tm = ts + AJ_RHS;
    double* sW = tm + AJ_RHS;
    const size_t bl = blockIdx.x, b = b0 + bl;
    const int l = blockIdx.y, L = gridDim.y;
    const double la = lam.v[l];
    const int nch = (int)((K + CH - 1) / CH);
    const size_t blk = (size_t)U * D;
    const double* pb = part + bl * (size_t)nchs * blk;
    const size_t i0 = (size_t)idx[b * ld];
    double* rf = rfit + (bl * L + l) * aj_rfit_dbl(nc, P);
    double* cb = rf + 1 + nc;               // (1 + nc) x P
    double* Mo = cb + (size_t)U * P;        // nc x nc
    for (int q = t; q < U; q += 256) {
        double s = 0.0;
        for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + q];
        if (q == 0) sW[0] = s; else xs[q - 1] = s;
    }
    __syncthreads();
    const double W = sW[0];
    if (t == 0) rf[0] = W;
    for (int k = t; k < nc; k += 256) {
        xm[k] = xs[k] / W;
        xb[k] = xm[k] + (aj_val(src, i0, k, nc) - O[b * KCO + k]);
        rf[1 + k] = xm[k];
    }
    __syncthreads();
    for (int q = t; q < nc * nc; q += 256) {
        const int k = q / nc, m = q % nc, lo = k < m ? k : m, hi = k < m ? m : k;
        double s = 0.0;
        for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + (size_t)(1 + lo) * D + 1 + hi];
        const double c = fma(-xm[lo], xs[hi], s);
        C0[q] = (k == m) ? fma(la, c, c) : c;
    }
    for (int j0 = 0; j0 == 0 || j0 < P; j0 += AJ_RHS) {
        const int nb = (P - j0 < AJ_RHS) ? P - j0 : AJ_RHS, NW = nc + nb;
        __syncthreads();
        for (int jj = t; jj < nb; jj += 256) {
            double s = 0.0;
            for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + 1 + nc + j0 + jj];
            ts[jj] = s;
            tm[jj] = aj_val(src, i0, nc + j0 + jj, nc) + s / W;
        }
        for (int q = t; q < nc * nc; q += 256) Wk[(q / nc) * NB + q % nc] = C0[q];
        __syncthreads();
        for (int q = t; q < nc * nb; q += 256) {
            const int k = q / nb, jj = q % nb;
            double s = 0.0;
            for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + (size_t)(1 + k) * D + 1 + nc + j0 + jj];
            Wk[k * NB + nc + jj] = fma(-xm[k], ts[jj], s);
        }
        __syncthreads();
        for (int k = 0; k < nc; k++) {
            const double d = Wk[k * NB + k], c0 = C0[k * nc + k];
            const bool keep = (c0 > 0.0) && (d > 1e-10 * c0);
            if (t == 0) kept[k] = keep ? 1.0 : 0.0;
            if (!keep) continue;                                // (uniform)
            for (int q = t; q < NW; q += 256) rowk[q] = (q == k) ? 1.0 / d : Wk[k * NB + q] / d;
            for (int i = t; i < nc; i += 256) colk[i] = Wk[i * NB + k];
            __syncthreads();
            for (int q = t; q < nc * NW; q += 256) {
                const int i = q / NW, j = q % NW;
                double v;
                if (i == k) v = rowk[j];
                else if (j == k) v = -colk[i] / d;
                else v = fma(-colk[i], rowk[j], Wk[i * NB + j]);
                Wk[i * NB + j] = v;
            }
            __syncthreads();
        }
        __syncthreads();
        if (j0 == 0)                                            // the left block is the same in every batch of right-hand sides
            for (int q = t; q < nc * nc; q += 256) {
                const int i = q / nc, j = q % nc;
                Mo[q] = (kept[i] != 0.0 && kept[j] != 0.0) ? Wk[i * NB + j] : 0.0;
            }
        for (int jj = t; jj < nb; jj += 256) {
            const int j = j0 + jj;
            double a = tm[jj];
            for (int k = 0; k < nc; k++) {
                const double be = (kept[k] != 0.0) ? Wk[k * NB + nc + jj] : 0.0;
                a = fma(-be, xb[k], a);
                cb[(size_t)(1 + k) * P + j] = be;
            }
            cb[j] = a;
        }
    }
}

// k_adj_press's tile: TR rows of [x (observation-centred) | theta] and, in one region used twice, M_l and then beta_l (when it
// fits AJ_APPLY_DBL: k_adj_apply's beta_lds rule); (nc, P) only
struct AjPlanR {
    int TR, beta_lds, reg;      // rows of a tile; beta_l in LDS; doubles of the shared region
    size_t lds;
};
constexpr int AJ_PRESS_DBL = 8192;                          // doubles of k_adj_press's LDS (64 KiB)

__host__ __device__ __forceinline__ AjPlanR aj_plan_r(int nc, int P) {
    AjPlanR r;
    const int Wv = nc + P, ncp = (nc + 1) & ~1;
    r.beta_lds = (nc * P <= AJ_APPLY_DBL) ? 1 : 0;
    int reg = nc * nc;
    if (r.beta_lds && nc * P > reg) reg = nc * P;
    r.reg = (reg + 1) & ~1;
    int tr = (AJ_PRESS_DBL - r.reg - 2 * ncp - 256 - 2) / (Wv + 2);
    if (tr > 256) tr = 256;
    r.TR = tr < 1 ? 1 : tr;
    r.lds = (size_t)(r.reg + 2 * ncp + 256 + 2 + r.TR * (Wv + 2)) * 8;
    return r;
}

// grid (tiles of TR rows, targets b0 + blockIdx.y, penalties): the leave-one-out terms of the tile's rows under penalty l.
// A lane owns rows for the leverage: xt = (x_e - x_0) - xm, s_k = sum_m M[k][m] xt[m] (an fma chain from 0.0, m ascending),
// q = sum_k xt[k] s_k (an fma chain from 0.0, k ascending), h_e = w_e (1 / W + q), den_e = 1 - h_e.  Then a thread owns (row,
// parameter) pairs: v = aj_adjusted with beta_l, r = v - alpha_l, u = r / den_e, the term w_e (u u), 0 for a row of weight 0.
// Then per parameter: NS = 256 / min(P, 256) threads, each the sum of every NS-th row's term ascending, those sums in thread
// order.  pp[((bl L + l) tiles + tile) P + j]; +inf in every j when a row of positive weight has den_e <= 1e-10 or NaN.
// RW: w_e = k_e om[i_e], as the moments (a row of om = 0 takes no part, as the Epanechnikov row at distance h).
template <bool RW>
__global__ __launch_bounds__(256) void k_adj_press(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist, size_t ld,
                                                   size_t K, int nc, int P, int kernel, const double* __restrict__ O, int KCO,
                                                   const double* __restrict__ rfit, size_t b0, double* __restrict__ pp,
                                                   const double* __restrict__ om) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ int s_inf;
    const AjPlanR pr = aj_plan_r(nc, P);
    const int t = threadIdx.x, Wv = nc + P, ncp = (nc + 1) & ~1, TR = pr.TR;
    double* reg = sm;                        // M_l, then beta_l
    double* xm = reg + pr.reg;               // nc
    double* x0 = xm + ncp;                   // nc: the first row's scores
    double* red = x0 + ncp;                  // 256
    double* wd = red + 256;                  // TR x 2: w_e, den_e
    double* tv = wd + 2 * (size_t)TR + 2;    // TR x Wv
    const size_t bl = blockIdx.y, b = b0 + bl, e0 = (size_t)blockIdx.x * TR;
    const int l = blockIdx.z, L = gridDim.z;
    const int nr = (K - e0 < (size_t)TR) ? (int)(K - e0) : TR;
    const uint64_t* ix = idx + b * ld;
    const double* dd = dist + b * ld;
    const double* rf = rfit + (bl * L + l) * aj_rfit_dbl(nc, P);
    const double* cf = rf + 1 + nc;          // alpha_l at [j], beta_l at [(1 + k) P + j]
    const double* Mg = cf + (size_t)(1 + nc) * P;
    const double W = rf[0];
    const double h = dd[K - 1];
    const bool rect = kernel == 1 || aj_fallback(dd, K);
    const size_t i0 = (size_t)ix[0];
    if (t == 0) s_inf = 0;
    for (int q = t; q < nc * nc; q += 256) reg[q] = Mg[q];
    for (int k = t; k < nc; k += 256) {
        xm[k] = rf[1 + k];
        x0[k] = aj_val(src, i0, k, nc);
    }
    for (int q = t; q < nr * Wv; q += 256) {
        const int r = q / Wv, c = q % Wv;
        tv[q] = aj_val(src, (size_t)ix[e0 + r], c, nc);     // raw: the scores are centred below
    }
    for (int r = t; r < nr; r += 256) wd[2 * r] = aj_weight_rw<RW>(dd[e0 + r], h, rect, om, RW ? (size_t)ix[e0 + r] : 0);
    __syncthreads();
    for (int r = t; r < nr; r += 256) {
        const double* x = tv + r * Wv;
        double q = 0.0;
        for (int k = 0; k < nc; k++) {
            double s = 0.0;
            for (int m = 0; m < nc; m++) s = fma(reg[k * nc + m], (x[m] - x0[m]) - xm[m], s);
            q = fma((x[k] - x0[k]) - xm[k], s, q);
        }
        const double w = wd[2 * r], den = 1.0 - w * (1.0 / W + q);
        wd[2 * r + 1] = den;
        if (w > 0.0 && !(den > 1e-10)) s_inf = 1;
    }
    __syncthreads();
    if (pr.beta_lds)
        for (int q = t; q < nc * P; q += 256) reg[q] = cf[P + q];
    for (int q = t; q < nr * nc; q += 256) {                    // x_e as k_adj_apply stages it
        const int r = q / nc, k = q % nc;
        tv[r * Wv + k] = tv[r * Wv + k] - O[b * KCO + k];
    }
    __syncthreads();
    const double* bt = pr.beta_lds ? reg : cf + P;
    for (int q = t; q < nr * P; q += 256) {                     // theta_e[j] -> its term (its own slot; the scores are only read)
        const int r = q / P, j = q % P;
        double* x = tv + r * Wv;
        const double w = wd[2 * r];
        double term = 0.0;
        if (w > 0.0) {
            const double v = aj_adjusted(x[nc + j], [&](int k) { return x[k]; }, bt + j, (size_t)P, nc);
            const double u = (v - cf[j]) / wd[2 * r + 1];
            term = w * (u * u);
        }
        x[nc + j] = term;
    }
    __syncthreads();
    const bool inf = s_inf != 0;
    double* po = pp + ((bl * L + l) * (size_t)gridDim.x + blockIdx.x) * (size_t)P;
    const int PW = P < 256 ? P : 256, NS = 256 / PW;
    const int j = t % PW, s = t / PW;
    for (int j0 = 0; j0 < P; j0 += PW) {
        const bool mine = s < NS && j0 + j < P;
        double a = 0.0;
        if (mine)
            for (int r = s; r < nr; r += NS) a += tv[r * Wv + nc + j0 + j];
        red[t] = a;
        __syncthreads();
        if (mine && s == 0) {
            for (int q = 1; q < NS; q++) a += red[q * PW + j];
            po[j0 + j] = inf ? __longlong_as_double(0x7ff0000000000000ll) : a;
        }
        __syncthreads();
    }
}

// where a regressing call under the ridge setting writes its record (the context's buffers)
struct AjRgOut {
    int32_t* pick;                  // slots x P
    double* press;                  // slots x L x P
    unsigned long long* unscored;   // device counter
    size_t rstride, roff;           // record slot = b rstride + roff (1, 0; a tolerance path, one tolerance per launch: T, t)
};

// one work-group per target b0 + blockIdx.x: PRESS_l[j] = the tiles' partials summed in tile order (NaN counts as +inf),
// pick[j] = the smallest l with the smallest PRESS (L - 1 and counted when every l is +inf), coef[b][:, j] = (alpha, beta) of the
// pick, rows above nc 0.  RW: a slot under the all-zero rule (W of its fits not positive) has every PRESS +inf, pick L - 1, every
// parameter counted as unscored, and keeps k_adj_solve's coef (NaN in rows 0 .. nc)
template <bool RW>
__global__ __launch_bounds__(256) void k_adj_pick(int nc, int P, int A, int L, int tiles, const double* __restrict__ rfit,
                                                  const double* __restrict__ pp, size_t b0, double* __restrict__ coef, AjRgOut ro) {
    __shared__ unsigned s_un;
    const int t = threadIdx.x;
    const size_t bl = blockIdx.x, b = b0 + bl, rs = b * ro.rstride + ro.roff;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    if (t == 0) s_un = 0;
    __syncthreads();
    double* cb = coef + b * (size_t)(A + 1) * P;
    if constexpr (RW) {
        if (!(rfit[bl * L * aj_rfit_dbl(nc, P)] > 0.0)) {           // (uniform)
            for (int j = t; j < P; j += 256) {
                for (int l = 0; l < L; l++) ro.press[(rs * L + l) * (size_t)P + j] = inf;
                ro.pick[rs * (size_t)P + j] = L - 1;
            }
            if (t == 0 && P > 0 && ro.unscored) atomicAdd(ro.unscored, (unsigned long long)P);
            return;
        }
    }
    for (int j = t; j < P; j += 256) {
        int best = L - 1;
        double pbest = inf;
        for (int l = 0; l < L; l++) {
            const double* q = pp + (bl * L + l) * (size_t)tiles * P + j;
            double s = 0.0;
            for (int tl = 0; tl < tiles; tl++) s += q[(size_t)tl * P];
            if (!(s < inf)) s = inf;
            ro.press[(rs * L + l) * (size_t)P + j] = s;
            if (s < pbest) {
                pbest = s;
                best = l;
            }
        }
        if (!(pbest < inf)) atomicAdd(&s_un, 1u);
        ro.pick[rs * (size_t)P + j] = best;
        const double* cf = rfit + (bl * L + best) * aj_rfit_dbl(nc, P) + 1 + nc;
        for (int k = 0; k <= nc; k++) cb[(size_t)k * P + j] = cf[(size_t)k * P + j];
        for (int k = nc; k < A; k++) cb[(size_t)(1 + k) * P + j] = 0.0;
    }
    __syncthreads();
    if (t == 0 && s_un && ro.unscored) atomicAdd(ro.unscored, (unsigned long long)s_un);
}

// grid (tiles of TR rows, targets b0 + blockIdx.y): theta[(b K + e) P + j] = theta_e[j] - sum_k beta_kj x_e[k] (one fma chain in k
// order), weight[b K + e] = w_e.  HC: the variance correction on top (aj_hcorr with the second fit hcoef, unless row 0 of the
// parameter holds the skip flag), before the back-transform
// RW: weight[b K + e] = k_e om[i_e]
template <bool HC, bool RW>
__global__ __launch_bounds__(256) void k_adj_apply(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist, size_t K,
                                                   int nc, int P, int A, int kernel, const double* __restrict__ O, int KCO,
                                                   const double* __restrict__ coef, int TR, int beta_lds, size_t b0, AbcTf tf,
                                                   double* __restrict__ theta, double* __restrict__ weight,
                                                   const double* __restrict__ hcoef, const double* __restrict__ om) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, Wv = nc + P;
    const size_t b = b0 + blockIdx.y, e0 = (size_t)blockIdx.x * TR;
    if (e0 >= K) return;
    const int nr = (K - e0 < (size_t)TR) ? (int)(K - e0) : TR;
    const uint64_t* ix = idx + b * K;
    const double* dd = dist + b * K;
    if (weight) {
        const double h = dd[K - 1];
        const bool rect = kernel == 1 || aj_fallback(dd, K);
        for (int r = t; r < nr; r += 256)
            weight[b * K + e0 + r] = aj_weight_rw<RW>(dd[e0 + r], h, rect, om, RW ? (size_t)ix[e0 + r] : 0);
    }
    if (!theta) return;
    if constexpr (RW) {
        // the all-zero rule without components: no NaN slope reaches the rows below, so the target's weights are looked at here
        // (nc > 0: k_adj_solve's NaN slopes make every row NaN)
        if (nc == 0) {                                              // (uniform)
            __shared__ int s_any;
            if (t == 0) s_any = 0;
            __syncthreads();
            const double h = dd[K - 1];
            const bool rect = kernel == 1 || aj_fallback(dd, K);
            int any = 0;
            for (size_t e = t; e < K; e += 256) any |= aj_weight_rw<true>(dd[e], h, rect, om, (size_t)ix[e]) > 0.0;
            if (any) s_any = 1;
            __syncthreads();
            if (!s_any) {
                for (int q = t; q < nr * P; q += 256) theta[(b * K + e0) * (size_t)P + q] = __longlong_as_double(0x7ff8000000000000ll);
                return;
            }
        }
    }
    const double* beta = coef + b * (size_t)(A + 1) * P + P;   // beta_kj at beta[k P + j]
    double* tv = sm;                                           // TR x Wv: [x (observation-centred) | theta]
    double* bl = sm + (((size_t)TR * Wv + 1) & ~(size_t)1);    // nc x P coefficients (beta_lds)
    if (beta_lds)
        for (int q = t; q < nc * P; q += 256) bl[q] = beta[q];
    for (int q = t; q < nr * Wv; q += 256) {
        const int r = q / Wv, c = q % Wv;
        const double v = aj_val(src, (size_t)ix[e0 + r], c, nc);
        tv[q] = (c < nc) ? v - O[b * KCO + c] : v;
    }
    __syncthreads();
    const double* bt = beta_lds ? bl : beta;
    for (int q = t; q < nr * P; q += 256) {
        const int r = q / P, j = q % P;
        const double* x = tv + r * Wv;
        double v = aj_adjusted(x[nc + j], [&](int k) { return x[k]; }, bt + j, (size_t)P, nc);
        if constexpr (HC) {
            const double* hc = hcoef + b * (size_t)(A + 1) * P + j;
            if (!isnan(hc[0])) v = aj_hcorr(v, beta[j - P], [&](int k) { return x[k]; }, hc + P, (size_t)P, nc);
        }
        theta[(b * K + e0 + r) * (size_t)P + j] = tf.kind ? tf_back_j(tf, j, v) : v;
    }
}

// out[i + ldo j] = forward (inverse: back) transform of V[i + ldv j] under parameter j's kind (tf.kind == NULL or kind 0: copied bit
// for bit).  Grid (row blocks, parameters), lanes along rows; in place is allowed (an element is read and written by one thread).
// A forward pass counts the entries of LOG / LOGIT columns outside their domain: one atomic add per work-group that found any.
__global__ __launch_bounds__(256) void k_tf_apply(AbcTf tf, const double* V, size_t ldv, size_t n, int inverse, double* out, size_t ldo,
                                                  unsigned long long* outside) {
    __shared__ unsigned red[256];
    const int t = threadIdx.x, j = (int)blockIdx.y;
    const int kind = tf.kind ? tf.kind[j] : 0;
    const double lo = kind == 2 ? tf.lo[j] : 0.0, hi = kind == 2 ? tf.hi[j] : 0.0;
    const double* v = V + ldv * (size_t)j;
    double* o = out + ldo * (size_t)j;
    unsigned cnt = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + t; i < n; i += (size_t)gridDim.x * 256) {
        const double y = v[i];
        const double r = inverse ? tf_back(kind, lo, hi, y) : tf_forward(kind, lo, hi, y);
        if (!inverse && kind != 0 && isnan(r)) cnt++;
        o[i] = r;
    }
    if (inverse || kind == 0 || !outside) return;                   // (uniform)
    red[t] = cnt;
    __syncthreads();
    for (int sft = 128; sft > 0; sft >>= 1) {
        if (t < sft) red[t] += red[t + sft];
        __syncthreads();
    }
    if (t == 0 && red[0]) atomicAdd(outside, (unsigned long long)red[0]);
}

struct AjPlan {
    size_t nch, CH;          // chunks of a target's rows and their size (K only)
    int TR;                  // rows of a k_adj_moments tile (nc, P only)
};

AjPlan aj_plan(size_t K, int nc, int P) {
    AjPlan p;
    const AjChunks ck = aj_chunks(K);
    p.nch = ck.nch;
    p.CH = ck.CH;
    const int D = 1 + nc + P, Ds = aj_stride(nc, P);
    int tr = (AJ_TILE_DBL - (D + 1) - 2) / (Ds + 1);
    if (tr > 128) tr = 128;                                 // (LDS for several work-groups per CU)
    if ((size_t)tr > p.CH) tr = (int)p.CH;
    p.TR = tr < 1 ? 1 : tr;
    return p;
}

// LDS bytes of k_adj_moments (TL = 1) and of k_adj_moments_path<TL> at tiles of TR rows: the first row, one weight column per
// tolerance lane, the rows (<= 60 KiB at TL = 1, <= 64.5 KiB at TL = 4)
size_t aj_moments_lds(int TR, int nc, int P, int TL) {
    const int D = 1 + nc + P;
    return (size_t)(((D + 1) & ~1) + TL * ((TR + 1) & ~1) + TR * aj_stride(nc, P)) * 8;
}

// k_adj_moments2's tile: the slot's coefficients in LDS up to AJ_APPLY_DBL doubles, the rows in what is left of AJ_TILE_DBL (the
// chains do not depend on the tile's rows)
struct AjPlan2 {
    int TR, cf_lds;
    size_t lds;
};

AjPlan2 aj_plan2(const AjPlan& pl, int nc, int P) {
    AjPlan2 q;
    const int D = 1 + nc + P, Ds = aj_stride(nc, P), ncf = (1 + nc) * P;
    q.cf_lds = ncf <= AJ_APPLY_DBL ? 1 : 0;
    int tr = (AJ_TILE_DBL - (D + 1) - 2 - (q.cf_lds ? ncf : 0)) / (Ds + 1);
    if (tr > 128) tr = 128;
    if ((size_t)tr > pl.CH) tr = (int)pl.CH;
    q.TR = tr < 1 ? 1 : tr;
    q.lds = (size_t)(((D + 1) & ~1) + ((q.TR + 1) & ~1) + q.TR * Ds + (q.cf_lds ? ncf : 0)) * 8;      // <= 60 KiB
    return q;
}

size_t aj_solve_lds(int nc) {
    const int NB = nc + AJ_RHS, ncp = (nc + 1) & ~1;
    return (size_t)(((nc * nc + 1) & ~1) + nc * NB + 5 * ncp + NB + 2 * AJ_RHS + 2) * 8;
}

size_t aj_ridge_tiles(size_t K, int nc, int P) {
    const AjPlanR pr = aj_plan_r(nc, P);
    return (K + pr.TR - 1) / pr.TR;
}

// The arena blocks of a regressing call, each with one byte count: aj_call_setup allocates with the fit's nc, aj_need counts with
// nc = A, its bound.
size_t aj_dist_bytes(size_t B, size_t K) { return B * K * 8; }                                        // (the caller's may be NULL)
size_t aj_coef_bytes(size_t slots, size_t A, size_t P) { return slots * (A + 1) * P * 8 + 8; }       // (the caller's may be NULL)
size_t aj_table_bytes(size_t N, size_t nc, size_t P) { return N * (nc + P) * 8; }                     // the row-major table
size_t aj_part_bytes(size_t K, size_t nc, size_t P) {    // one target's moment blocks
    return aj_plan(K, 0, 0).nch * (1 + nc) * (1 + nc + P) * 8;
}
size_t aj_part2_bytes(size_t K, size_t nc, size_t P) {   // ... its second-stage blocks (the variance correction)
    return aj_plan(K, 0, 0).nch * (1 + nc) * P * 8;
}
size_t aj_rfit_bytes(size_t nc, size_t P, size_t L) { return L * aj_rfit_dbl((int)nc, (int)P) * 8; }  // ... its penalised fits
size_t aj_rpp_bytes(size_t K, size_t nc, size_t P, size_t L) {                                        // ... and their PRESS partials
    return L * aj_ridge_tiles(K, (int)nc, (int)P) * P * 8;
}

// targets per batch: the moment blocks of a batch, T sets of them on a tolerance path, within AJ_PART_BYTES (from A, an upper
// bound of nc, so that the arena bound does not depend on the fit)
size_t aj_batch(size_t K, size_t A, size_t P, size_t B, size_t T) {
    size_t bb = AJ_PART_BYTES / (T * aj_part_bytes(K, A, P));
    if (bb < 1) bb = 1;
    if (bb > AJ_MAX_GRID_Y) bb = AJ_MAX_GRID_Y;
    return bb < B ? bb : B;
}

// the table when the retained rows outnumber N / 4 (measured: DESIGN.md 7b) and it is not too large; decided from A (an upper bound
// of nc) so that the arena bound does not depend on the fit.  Diagnostic switch ABC_ADJ_GATHER=table / direct (ABC_DIAG=1).
bool aj_use_table(size_t N, size_t A, size_t P, size_t B, size_t K) {
    if (N * (A + P) * 8 > AJ_TABLE_MAX_BYTES) return false;
    if (const char* e = abc_diag_env("ABC_ADJ_GATHER")) {
        if (!strcmp(e, "table")) return true;
        if (!strcmp(e, "direct")) return false;
    }
    return 4 * B * K >= N;
}

// the bound of what aj_call_setup takes from the arena, block for block (T = 1: the adjust call; 256 per block for the alignment)
size_t aj_need(size_t N, size_t A, size_t P, size_t B, size_t K, size_t T, bool hcorr, size_t ridge) {
    const size_t bb = aj_batch(K, A, P, B, T);
    size_t b = aj_dist_bytes(B, K) + aj_coef_bytes(B * T, A, P);
    if (aj_use_table(N, A, P, B, K)) b += aj_table_bytes(N, A, P);
    b += bb * T * aj_part_bytes(K, A, P);
    if (hcorr) b += bb * aj_part2_bytes(K, A, P) + 256;
    if (ridge) b += bb * (aj_rfit_bytes(A, P, ridge) + aj_rpp_bytes(K, A, P, ridge)) + 2 * 256;
    return b + 16 * 256;
}

// What does not change within a regressing call: everything the fit chain takes besides the tolerance, the targets and the slot
struct AjCall {
    AjSrc src;
    const uint64_t* idx;
    const double* d;                        // the retained rows' distances, laid out as idx
    int nc, P, A, kernel;
    const double* O;                        // the targets' scores, O[b KCO + k]
    int KCO;
    const double* om;                       // row importance weights (NULL: none, and the instances below are the RW = false ones,
                                            // which ran before the setting existed)
    decltype(&k_adj_moments<false>) moments;
    decltype(&k_adj_moments2<false>) moments2;
    decltype(&k_adj_solve<false, false>) solve, solve_hc;
    decltype(&k_adj_press<false>) press;
    decltype(&k_adj_pick<false>) pick;
    size_t lds_s;                           // LDS bytes of k_adj_solve and k_adj_rsolve
    double* coef;                           // the call's coef, slots x (A + 1) x P
    double* part;                           // moment blocks of one batch
    double *hcoef, *part2;                  // the variance correction: its record (NULL: off), second-stage blocks of one batch
    unsigned long long* skipped;
    AbcRg rg;                               // ridge: the penalties and the record (L == 0: off)
    AjLam lam;
    double *rfit, *rpp;                     // ... the penalised fits and PRESS partials of one batch
};

// The set-up of a regressing call, after its ranking: nc from the model header (the call's one stream synchronisation), coef, the
// rows' source with the table when aj_use_table says so, the kernel instances, and the blocks of one batch of bb targets (T sets
// of moment blocks on a path) with those of the settings that are on; keep (if given) is filled for the products.
int aj_call_setup(abc_ctx* ctx, const char* fn, const abc_tg_scores& sc, const double* Y, size_t ldy, size_t N, size_t P,
                  const double* model, size_t A, size_t B, size_t K, size_t T, size_t bb, int kernel, const uint64_t* idx, const double* d,
                  double* coef, const AbcTf& tf, const AbcHc* hc, const AbcRg* rg, const double* om, abc_adj_keep* keep, AjCall* c) {
    double hdr = 0.0;
    ABC_HIP(ctx, hipMemcpyAsync(&hdr, model, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int nc = hdr < 0.0 ? 0 : (hdr > (double)A ? (int)A : (int)hdr);      // the ranking's tg_ncomp
    const int Pi = (int)P;
    *c = AjCall{};
    c->idx = idx;
    c->d = d;
    c->nc = nc;
    c->P = Pi;
    c->A = (int)A;
    c->kernel = kernel;
    c->O = sc.O;
    c->KCO = sc.KCO;
    c->om = om;
    c->coef = coef ? coef : (double*)abc_ws_alloc(ctx, aj_coef_bytes(B * T, A, P));
    if (!c->coef) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);

    c->src = AjSrc{nullptr, (size_t)nc + P, sc.S, sc.sld, Y, ldy};
    if (aj_use_table(N, A, P, B, K) && c->src.W > 0) {
        double* Tb = (double*)abc_ws_alloc(ctx, aj_table_bytes(N, (size_t)nc, P));
        if (!Tb) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        size_t blocks = (N + 63) / 64;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(k_adj_table, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, sc.S, sc.sld, Y, ldy, N, nc, Pi, Tb);
        ABC_HIP(ctx, hipGetLastError());
        c->src.T = Tb;
    }

    // under row importance weights every kernel that makes or sums weights is its RW instance
    c->moments = om ? k_adj_moments<true> : k_adj_moments<false>;
    c->moments2 = om ? k_adj_moments2<true> : k_adj_moments2<false>;
    c->solve = om ? k_adj_solve<false, true> : k_adj_solve<false, false>;
    c->solve_hc = om ? k_adj_solve<true, true> : k_adj_solve<true, false>;
    c->press = om ? k_adj_press<true> : k_adj_press<false>;
    c->pick = om ? k_adj_pick<true> : k_adj_pick<false>;
    c->lds_s = aj_solve_lds(nc);
    ABC_HIP(ctx, hipFuncSetAttribute((const void*)c->solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_s));
    c->part = (double*)abc_ws_alloc(ctx, bb * T * aj_part_bytes(K, (size_t)nc, P));
    if (!c->part) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    if (hc && Pi > 0) {                                                // the variance correction: a second fit after every first
        c->hcoef = hc->hcoef;
        c->skipped = hc->skipped;
        c->part2 = (double*)abc_ws_alloc(ctx, bb * aj_part2_bytes(K, (size_t)nc, P));
        if (!c->part2) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        ABC_HIP(ctx, hipFuncSetAttribute((const void*)c->solve_hc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_s));
    }
    if (rg && rg->L > 0 && Pi > 0) {                                   // ridge: the penalised fits replace every first fit's coef
        c->rg = *rg;
        for (int l = 0; l < rg->L; l++) c->lam.v[l] = rg->lambda[l];
        c->rfit = (double*)abc_ws_alloc(ctx, bb * aj_rfit_bytes((size_t)nc, P, (size_t)rg->L));
        c->rpp = (double*)abc_ws_alloc(ctx, bb * aj_rpp_bytes(K, (size_t)nc, P, (size_t)rg->L));
        if (!c->rfit || !c->rpp) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        ABC_HIP(ctx, hipFuncSetAttribute((const void*)k_adj_rsolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_s));
        ABC_HIP(ctx, hipFuncSetAttribute((const void*)c->press, hipFuncAttributeMaxDynamicSharedMemorySize, (int)aj_plan_r(nc, Pi).lds));
    }
    if (keep) *keep = abc_adj_keep{c->src, sc.O, sc.KCO, nc, c->coef, d, tf, c->hcoef};
    return ABC_OK;
}

// The fit of abc_rank_targets_adjust_dev at one tolerance for the targets b0 .. b0 + nb - 1: the first K of a target's ld retained
// rows, in the chunks of pl = aj_plan(K, ..).  k_adj_moments and k_adj_solve give coef (and rank / status where given) at slot
// b; under ridge k_adj_rsolve, k_adj_press and k_adj_pick replace that coef before anything reads it; under the variance
// correction k_adj_moments2 and k_adj_solve<true> fit its residuals.  The settings' records (pick, press, hcoef) go to slot
// b sstride + soff: (1, 0) for the adjust call, (T, t) for tolerance t of a path, whose coef is not laid out as the chain's;
// for it the picked fit is also copied to that slot of slot_coef, right behind the pick (NULL: no copy).
// Both entries fit through this one function, so a path's records at (b, t) have the bits of the adjust call with K = K_t.
int aj_fit_chain(abc_ctx* ctx, const AjCall& c, const AjPlan& pl, size_t ld, size_t K, size_t b0, size_t nb, size_t sstride,
                 size_t soff, double* coef, int32_t* rank, int32_t* status, double* slot_coef) {
    AjKs ks = {};
    ks.K[0] = K;
    const AjHcSolve hs0 = {nullptr, nullptr, nullptr, nullptr, 1, 0};
    hipLaunchKernelGGL(c.moments, dim3((unsigned)pl.nch, (unsigned)nb), dim3(256), aj_moments_lds(pl.TR, c.nc, c.P, 1), ctx->stream,
                       c.src, c.idx, c.d, ld, K, c.nc, c.P, c.kernel, pl.CH, pl.TR, b0, pl.nch, c.part, c.om);
    hipLaunchKernelGGL(c.solve, dim3((unsigned)nb), dim3(256), c.lds_s, ctx->stream, c.src, c.idx, c.d, ld, ks, 1, pl.CH, c.nc, c.P,
                       c.A, c.kernel, c.O, c.KCO, (const double*)c.part, (int)pl.nch, b0, coef, rank, status, hs0);
    ABC_HIP(ctx, hipGetLastError());
    if (c.rg.L > 0) {
        const AjPlanR pr = aj_plan_r(c.nc, c.P);
        const size_t tiles = aj_ridge_tiles(K, c.nc, c.P);
        const AjRgOut ro = {c.rg.pick, c.rg.press, c.rg.unscored, sstride, soff};
        hipLaunchKernelGGL(k_adj_rsolve, dim3((unsigned)nb, (unsigned)c.rg.L), dim3(256), c.lds_s, ctx->stream, c.src, c.idx, ld, K,
                           pl.CH, c.nc, c.P, c.O, c.KCO, (const double*)c.part, (int)pl.nch, b0, c.lam, c.rfit);
        hipLaunchKernelGGL(c.press, dim3((unsigned)tiles, (unsigned)nb, (unsigned)c.rg.L), dim3(256), pr.lds, ctx->stream, c.src,
                           c.idx, c.d, ld, K, c.nc, c.P, c.kernel, c.O, c.KCO, (const double*)c.rfit, b0, c.rpp, c.om);
        hipLaunchKernelGGL(c.pick, dim3((unsigned)nb), dim3(256), 0, ctx->stream, c.nc, c.P, c.A, c.rg.L, (int)tiles,
                           (const double*)c.rfit, (const double*)c.rpp, b0, coef, ro);
        ABC_HIP(ctx, hipGetLastError());
        if (slot_coef) {
            const size_t cn = (size_t)(c.A + 1) * c.P, cw = cn * 8;
            ABC_HIP(ctx, hipMemcpy2DAsync(slot_coef + (b0 * sstride + soff) * cn, sstride * cw, coef + b0 * cn, cw, cw, nb,
                                          hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    if (!c.hcoef) return ABC_OK;
    const AjPlan2 p2 = aj_plan2(pl, c.nc, c.P);
    const AjHcSolve hs1 = {c.part2, coef, c.hcoef, c.skipped, sstride, soff};
    hipLaunchKernelGGL(c.moments2, dim3((unsigned)pl.nch, (unsigned)nb), dim3(256), p2.lds, ctx->stream, c.src, c.idx, c.d, ld, K,
                       c.nc, c.P, c.A, c.kernel, pl.CH, p2.TR, b0, pl.nch, c.O, c.KCO, (const double*)coef, 1, 0, p2.cf_lds, c.part2,
                       c.om);
    hipLaunchKernelGGL(c.solve_hc, dim3((unsigned)nb), dim3(256), c.lds_s, ctx->stream, c.src, c.idx, c.d, ld, ks, 1, pl.CH, c.nc,
                       c.P, c.A, c.kernel, c.O, c.KCO, (const double*)c.part, (int)pl.nch, b0, (double*)nullptr, (int32_t*)nullptr,
                       (int32_t*)nullptr, hs1);
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

template <int TL>
int aj_launch_moments_path(abc_ctx* ctx, const AjCall& c, size_t ld, const AjKs& ks, int T, int t0, const AjPlan& pl, size_t b0,
                           size_t nb) {
    const size_t lds = aj_moments_lds(pl.TR, c.nc, c.P, TL);
    const auto mp = c.om ? k_adj_moments_path<TL, true> : k_adj_moments_path<TL, false>;
    ABC_HIP(ctx, hipFuncSetAttribute((const void*)mp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mp, dim3((unsigned)pl.nch, (unsigned)nb), dim3(256), lds, ctx->stream, c.src, c.idx, c.d, ld, ks, T, t0, c.nc,
                       c.P, c.kernel, pl.CH, pl.TR, b0, pl.nch, c.part, c.om);
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

}  // namespace

size_t abc_adjust_need(size_t N, size_t A, size_t P, size_t B, size_t K, bool hcorr, size_t ridge) {
    return aj_need(N, A, P, B, K, 1, hcorr, ridge) + 2 * B * 4;      // (rank, status: the caller's; kept in the bound)
}

int launch_rank_targets_adjust(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                               const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                               bool any_excl, size_t K, int kernel, uint64_t* idx, double* dist, const abc_adjust_out* out,
                               abc_adj_keep* keep, const AbcTf* tf, const AbcHc* hc, const AbcRg* rg, const double* om) {
    const AbcTf tfd = tf ? *tf : AbcTf{nullptr, nullptr, nullptr};
    double* d = dist ? dist : (double*)abc_ws_alloc(ctx, aj_dist_bytes(B, K));
    if (!d) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets_adjust: workspace exhausted");
    abc_tg_scores sc;
    ABC_TRY(launch_rank_targets(ctx, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, any_excl, K, idx, d, nullptr, &sc));
    if (!keep && !out->theta && !out->weight && !out->coef && !out->rank && !out->status) return ABC_OK;

    const size_t bb = aj_batch(K, A, P, B, 1);
    AjCall c;
    ABC_TRY(aj_call_setup(ctx, "rank_targets_adjust", sc, Y, ldy, N, P, model, A, B, K, 1, bb, kernel, idx, d, out->coef, tfd, hc, rg,
                          om, keep, &c));
    const int nc = c.nc, Pi = c.P;
    const AjPlan pl = aj_plan(K, nc, Pi);
    for (size_t b0 = 0; b0 < B; b0 += bb)
        ABC_TRY(aj_fit_chain(ctx, c, pl, K, K, b0, (B - b0 < bb) ? B - b0 : bb, 1, 0, c.coef, out->rank, out->status, nullptr));

    if (out->theta || out->weight) {
        const int Wv = nc + Pi;
        int TR = Wv > 0 ? AJ_APPLY_DBL / Wv : 64;
        if (TR > 64) TR = 64;
        if (TR < 1) TR = 1;
        const int beta_lds = (nc * Pi <= AJ_APPLY_DBL) ? 1 : 0;
        const size_t lds_a = (size_t)((((size_t)TR * Wv + 1) & ~(size_t)1) + (beta_lds ? (size_t)nc * Pi : 0)) * 8;     // <= 64 KiB
        const auto apply = om ? (c.hcoef ? k_adj_apply<true, true> : k_adj_apply<false, true>)
                              : (c.hcoef ? k_adj_apply<true, false> : k_adj_apply<false, false>);
        ABC_HIP(ctx, hipFuncSetAttribute((const void*)apply, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
        const size_t tiles = (K + TR - 1) / TR;
        for (size_t b0 = 0; b0 < B; b0 += AJ_MAX_GRID_Y) {
            const size_t nb = (B - b0 < AJ_MAX_GRID_Y) ? B - b0 : AJ_MAX_GRID_Y;
            hipLaunchKernelGGL(apply, dim3((unsigned)tiles, (unsigned)nb), dim3(256), lds_a, ctx->stream, c.src, (const uint64_t*)idx,
                               (const double*)d, K, nc, Pi, (int)A, kernel, sc.O, sc.KCO, (const double*)c.coef, TR, beta_lds, b0,
                               tfd, out->theta, out->weight, (const double*)c.hcoef, om);
            ABC_HIP(ctx, hipGetLastError());
        }
    }
    return ABC_OK;
}

size_t abc_path_need(size_t N, size_t A, size_t P, size_t B, size_t K, size_t T, bool hcorr, size_t ridge) {
    size_t b = aj_need(N, A, P, B, K, T, hcorr, ridge);
    if (hcorr || ridge) b += aj_coef_bytes(B, A, P) + 2 * 256;       // the refits' coef
    return b;
}

int launch_rank_targets_path(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                             const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                             bool any_excl, int kernel, uint64_t* idx, double* dist, const abc_path* path, abc_adj_keep* keep,
                             const double* Yt, const AbcTf* tf, const AbcHc* hc, const AbcRg* rg, const double* om) {
    const int T = (int)path->T, Pi = (int)P;
    AjKs ks = {};
    for (int t = 0; t < T; t++) ks.K[t] = path->Ks[t];
    const size_t K = ks.K[T - 1];                                    // K_max: the ranking's K and the rows' stride
    double* d = dist ? dist : (double*)abc_ws_alloc(ctx, aj_dist_bytes(B, K));
    if (!d) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets_path: workspace exhausted");
    abc_tg_scores sc;
    ABC_TRY(launch_rank_targets(ctx, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, any_excl, K, idx, d, nullptr, &sc));
    const bool fit = path->coef || path->rank || path->status || keep;
    if (!fit && !path->post_mean && !path->h) return ABC_OK;

    const AjSrc raw = {nullptr, P, nullptr, 0, Y, ldy};              // the parameters only: post_mean is of the raw Y under transforms too
    AjCall c = {};
    c.src = raw;                                                     // (all k_path_mean reads without the fit)
    if (fit) {
        // the fit on the transformed scale reads Yt (N x P, ld = N); the table by the adjustment's rule with K = K_max
        const size_t bb = aj_batch(K, A, P, B, (size_t)T);
        ABC_TRY(aj_call_setup(ctx, "rank_targets_path", sc, Yt ? Yt : Y, Yt ? N : ldy, N, P, model, A, B, K, (size_t)T, bb, kernel, idx,
                              d, path->coef, (Yt && tf) ? *tf : AbcTf{nullptr, nullptr, nullptr}, hc, rg, om, keep, &c));
        const int nc = c.nc;
        const bool refit = c.hcoef || c.rg.L > 0;
        double* coef1 = refit ? (double*)abc_ws_alloc(ctx, aj_coef_bytes(B, A, P)) : nullptr;
        if (refit && !coef1) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets_path: workspace exhausted");
        const AjPlan pl = aj_plan(K, nc, Pi);
        const size_t blk = (size_t)(1 + nc) * (1 + nc + P);
        const bool wide = (1 + nc + Pi) * ((1 + nc + 3) / 4) > 256;  // more than 256 entry groups: k_adj_moments, once per tolerance
        const AjHcSolve hs0 = {nullptr, nullptr, nullptr, nullptr, 1, 0};
        for (size_t b0 = 0; b0 < B; b0 += bb) {
            const size_t nb = (B - b0 < bb) ? B - b0 : bb;
            if (wide) {
                for (int t = 0; t < T; t++) {
                    const size_t ncht = (ks.K[t] + pl.CH - 1) / pl.CH;
                    hipLaunchKernelGGL(c.moments, dim3((unsigned)ncht, (unsigned)nb), dim3(256), aj_moments_lds(pl.TR, nc, Pi, 1),
                                       ctx->stream, c.src, (const uint64_t*)idx, (const double*)d, K, ks.K[t], nc, Pi, kernel, pl.CH,
                                       pl.TR, b0, (size_t)T * pl.nch, c.part + (size_t)t * pl.nch * blk, om);
                }
                ABC_HIP(ctx, hipGetLastError());
            } else {
                // passes of at most 4 tolerance lanes, from the largest down (8 lanes take 256 VGPRs on gfx950: one work-group per CU)
                for (int hi = T; hi > 0;) {
                    const int n = hi < 4 ? hi : 4, TL = n > 2 ? 4 : n, t0 = hi - TL;
                    switch (TL) {
                    case 1: ABC_TRY(aj_launch_moments_path<1>(ctx, c, K, ks, T, t0, pl, b0, nb)); break;
                    case 2: ABC_TRY(aj_launch_moments_path<2>(ctx, c, K, ks, T, t0, pl, b0, nb)); break;
                    default: ABC_TRY(aj_launch_moments_path<4>(ctx, c, K, ks, T, t0, pl, b0, nb)); break;
                    }
                    hi -= n;
                }
            }
            hipLaunchKernelGGL(c.solve, dim3((unsigned)nb, (unsigned)T), dim3(256), c.lds_s, ctx->stream, c.src, (const uint64_t*)idx,
                               (const double*)d, K, ks, T, pl.CH, nc, Pi, (int)A, kernel, sc.O, sc.KCO, (const double*)c.part,
                               (int)pl.nch, b0, c.coef, path->rank, path->status, hs0);
            ABC_HIP(ctx, hipGetLastError());
            // Under the variance correction or ridge, tolerance t then goes through the adjust call's own chain with K = K_t, in
            // that call's chunks (aj_plan(K_t, ..): never more chunks than pl's, so `part` holds them once the solve above has
            // read it), one tolerance at a time.  coef1 is that call's coef: it differs from the path's in the last bits where the
            // chunks of K_max and of K_t differ.  Under ridge it is the picked fit, which the chain copies to slot (b, t) of the
            // path's coef (rank and status stay the path's own); the second fit models coef1's residuals, and slot (b, t) of
            // hcoef, pick and press is the chain's record at (T, t).
            for (int t = 0; refit && t < T; t++)
                ABC_TRY(aj_fit_chain(ctx, c, aj_plan(ks.K[t], nc, Pi), K, ks.K[t], b0, nb, (size_t)T, (size_t)t, coef1, nullptr, nullptr,
                                     c.rg.L > 0 ? c.coef : nullptr));
        }
    }
    if (path->post_mean || path->h) {
        const size_t step = (size_t)1 << 30;
        for (size_t b0 = 0; b0 < B; b0 += step) {
            const size_t nb = (B - b0 < step) ? B - b0 : step;
            hipLaunchKernelGGL(om ? k_path_mean<true> : k_path_mean<false>, dim3((unsigned)nb, (unsigned)T), dim3(256), 0, ctx->stream,
                               Yt ? raw : c.src, c.nc, (const uint64_t*)idx + b0 * K, (const double*)d + b0 * K, K, ks, T, Pi,
                               path->post_mean ? path->post_mean + b0 * T * P : nullptr, path->h ? path->h + b0 * T : nullptr, om);
            ABC_HIP(ctx, hipGetLastError());
        }
    }
    return ABC_OK;
}

int launch_param_transf(abc_ctx* ctx, const AbcTf* tf, const double* V, size_t ldv, size_t n, size_t P, int inverse, double* out,
                        size_t ldo, unsigned long long* outside) {
    if (n == 0 || P == 0) return ABC_OK;
    size_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const AbcTf tfd = tf ? *tf : AbcTf{nullptr, nullptr, nullptr};
    for (size_t j0 = 0; j0 < P; j0 += AJ_MAX_GRID_Y) {
        const size_t np = (P - j0 < AJ_MAX_GRID_Y) ? P - j0 : AJ_MAX_GRID_Y;
        AbcTf tj = tfd;
        if (tj.kind) { tj.kind += j0; tj.lo += j0; tj.hi += j0; }
        hipLaunchKernelGGL(k_tf_apply, dim3((unsigned)blocks, (unsigned)np), dim3(256), 0, ctx->stream, tj, V + ldv * j0, ldv, n, inverse,
                           out + ldo * j0, ldo, outside);
        ABC_HIP(ctx, hipGetLastError());
    }
    return ABC_OK;
}

static_assert(AJ_MAXA == 64 && AJ_MAXP == 1024, "limits of abc_rank_targets_adjust_dev (api.hip checks them)");
static_assert(sizeof(AbcRg::lambda) == ABC_RIDGE_MAXL * sizeof(double), "AbcRg holds ABC_RIDGE_MAXL penalties");
