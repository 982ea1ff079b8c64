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

// grid (chunks, targets b0 + blockIdx.y); part[((blockIdx.y nch + chunk) U + r) D + c] = sum over the chunk's rows e (ascending) of
// (w_e u_r) v_c, u = [1, x'], v = [1, x', theta'], x' / theta' = the row's values minus those of the target's first row.  Rows are
// staged TR at a time.  A thread owns one group of four entries when the block has at most 256 groups and keeps their sums in
// registers; otherwise an entry's running sum passes between tiles through part.  The chain is the same either way and for every TR.
__global__ __launch_bounds__(256) void k_adj_moments(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist,
                                                     size_t K, int nc, int P, int kernel, size_t CH, int TR, size_t b0,
                                                     double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x;
    const int U = 1 + nc, D = 1 + nc + P, Wv = nc + P, Ds = aj_stride(nc, P);
    const int Dp = (D + 1) & ~1, TRp = (TR + 1) & ~1;
    double* shift = sm;                  // [1 + c]: the first row's value c
    double* tw = sm + Dp;                // TR weights
    double* tv = tw + TRp;               // TR x Ds
    const size_t b = b0 + blockIdx.y, nch = gridDim.x, chunk = blockIdx.x;
    const uint64_t* ix = idx + b * K;
    const double* dd = dist + b * K;
    const size_t e0 = chunk * CH, e1 = (e0 + CH < K) ? e0 + CH : K;
    const double h = dd[K - 1];
    const bool rect = kernel == 1 || aj_fallback(dd, K);
    const size_t i0 = (size_t)ix[0];
    for (int c = t; c < Wv; c += 256) shift[1 + c] = aj_val(src, i0, c, nc);
    double* pp = part + ((size_t)blockIdx.y * nch + chunk) * (size_t)U * D;
    const int nrg = (U + 3) / 4, J = D * nrg;
    const bool regs = J <= 256;
    double racc[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t r0 = e0; r0 < e1; r0 += (size_t)TR) {
        const int nr = (e1 - r0 < (size_t)TR) ? (int)(e1 - r0) : TR;
        __syncthreads();                                        // the shift is written, the previous tile consumed
        for (int q = t; q < nr * Wv; q += 256) {
            const int r = q / Wv, c = q % Wv;
            tv[r * Ds + 1 + c] = aj_val(src, (size_t)ix[r0 + r], c, nc) - shift[1 + c];
        }
        for (int r = t; r < nr; r += 256) {
            tv[r * Ds] = 1.0;
            for (int c = D; c < Ds; c++) tv[r * Ds + c] = 0.0;
            tw[r] = aj_weight(dd[r0 + r], h, rect);
        }
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

// one work-group per target b0 + blockIdx.x: the moments (chunks summed in order), centred; the sweep; coef, rank and status
__global__ __launch_bounds__(256) void k_adj_solve(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist,
                                                   size_t K, int nc, int P, int A, int kernel, const double* __restrict__ O, int KCO,
                                                   const double* __restrict__ part, int nch, size_t b0, double* __restrict__ coef,
                                                   int32_t* __restrict__ rank, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
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
    const size_t bl = blockIdx.x, b = b0 + bl;
    const size_t blk = (size_t)U * D;
    const double* pb = part + bl * (size_t)nch * blk;
    const size_t i0 = (size_t)idx[b * K];
    for (int q = t; q < U; q += 256) {
        double s = 0.0;
        for (int ch = 0; ch < nch; ch++) s += pb[ch * blk + q];
        if (q == 0) sW[0] = s; else xs[q - 1] = s;
    }
    __syncthreads();
    const double W = sW[0];
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
    double* cb = coef + b * (size_t)(A + 1) * P;
    for (int j0 = 0; j0 == 0 || j0 < P; j0 += AJ_RHS) {
        const int nb = (P - j0 < AJ_RHS) ? P - j0 : AJ_RHS, NW = nc + nb;
        __syncthreads();                                        // C0 written, the previous batch's coefficients read
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
        for (int jj = t; jj < nb; jj += 256) {
            const int j = j0 + jj;
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
    if (t == 0) {
        int r = 0;
        for (int k = 0; k < nc; k++) r += kept[k] != 0.0;
        if (rank) rank[b] = r;
        if (status) status[b] = (r < nc ? 1 : 0) | ((kernel == 0 && aj_fallback(dist + b * K, K)) ? 2 : 0);
    }
}

// grid (tiles of TR rows, targets b0 + blockIdx.y): theta[(b K + e) P + j] = theta_e[j] - sum_k beta_kj x_e[k] (one fma chain in k
// order), weight[b K + e] = w_e
__global__ __launch_bounds__(256) void k_adj_apply(AjSrc src, const uint64_t* __restrict__ idx, const double* __restrict__ dist, size_t K,
                                                   int nc, int P, int A, int kernel, const double* __restrict__ O, int KCO,
                                                   const double* __restrict__ coef, int TR, int beta_lds, size_t b0,
                                                   double* __restrict__ theta, double* __restrict__ weight) {
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
        for (int r = t; r < nr; r += 256) weight[b * K + e0 + r] = aj_weight(dd[e0 + r], h, rect);
    }
    if (!theta) return;
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
        theta[(b * K + e0 + r) * (size_t)P + j] = aj_adjusted(x[nc + j], [&](int k) { return x[k]; }, bt + j, (size_t)P, nc);
    }
}

struct AjPlan {
    size_t nch, CH;          // chunks of a target's rows and their size (K only)
    int TR;                  // rows of a k_adj_moments tile (nc, P only)
};

AjPlan aj_plan(size_t K, int nc, int P) {
    AjPlan p;
    p.nch = (K + 255) / 256;
    if (p.nch > 64) p.nch = 64;
    p.CH = (K + p.nch - 1) / p.nch;
    p.nch = (K + p.CH - 1) / p.CH;
    const int D = 1 + nc + P, Ds = aj_stride(nc, P);
    int tr = (AJ_TILE_DBL - (D + 1) - 2) / (Ds + 1);
    if (tr > 128) tr = 128;                                 // (LDS for several work-groups per CU)
    if ((size_t)tr > p.CH) tr = (int)p.CH;
    p.TR = tr < 1 ? 1 : tr;
    return p;
}

size_t aj_part_bytes(size_t K, size_t A, size_t P) {     // one target's moment blocks (bound over nc <= A)
    const AjPlan p = aj_plan(K, 0, 0);
    return p.nch * (1 + A) * (1 + A + P) * 8;
}

size_t aj_batch(size_t K, size_t A, size_t P, size_t B) {
    size_t bb = AJ_PART_BYTES / aj_part_bytes(K, A, P);
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

size_t aj_solve_lds(int nc) {
    const int NB = nc + AJ_RHS, ncp = (nc + 1) & ~1;
    return (size_t)(((nc * nc + 1) & ~1) + nc * NB + 5 * ncp + NB + 2 * AJ_RHS + 2) * 8;
}

}  // namespace

size_t abc_adjust_need(size_t N, size_t A, size_t P, size_t B, size_t K) {
    size_t b = 0;
    b += B * K * 8;                                          // distances (the caller's may be NULL)
    b += B * (A + 1) * P * 8 + 2 * B * 4;                    // coefficients, rank, status
    if (aj_use_table(N, A, P, B, K)) b += N * (A + P) * 8;   // the row-major table
    b += aj_batch(K, A, P, B) * aj_part_bytes(K, A, P);      // moment blocks of one batch
    return b + 16 * 256;
}

int launch_rank_targets_adjust(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                               const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                               bool any_excl, size_t K, int kernel, uint64_t* idx, double* dist, const abc_adjust_out* out,
                               abc_adj_keep* keep) {
    double* d = dist ? dist : (double*)abc_ws_alloc(ctx, B * K * 8);
    if (!d) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets_adjust: workspace exhausted");
    abc_tg_scores sc;
    ABC_TRY(launch_rank_targets(ctx, X, ldx, Y, ldy, N, M, P, model, A, targets, ldt, B, exclude, any_excl, K, idx, d, nullptr, &sc));
    if (!keep && !out->theta && !out->weight && !out->coef && !out->rank && !out->status) return ABC_OK;

    double hdr = 0.0;
    ABC_HIP(ctx, hipMemcpyAsync(&hdr, model, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int nc = hdr < 0.0 ? 0 : (hdr > (double)A ? (int)A : (int)hdr);      // the ranking's tg_ncomp
    const int Pi = (int)P;
    double* coef = out->coef ? out->coef : (double*)abc_ws_alloc(ctx, B * (A + 1) * P * 8 + 8);
    if (!coef) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets_adjust: workspace exhausted");

    AjSrc src;
    src.T = nullptr;
    src.W = (size_t)nc + P;
    src.S = sc.S;
    src.sld = sc.sld;
    src.Y = Y;
    src.ldy = ldy;
    if (aj_use_table(N, A, P, B, K) && src.W > 0) {
        double* T = (double*)abc_ws_alloc(ctx, N * src.W * 8);
        if (!T) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets_adjust: workspace exhausted");
        size_t blocks = (N + 63) / 64;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(k_adj_table, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, sc.S, sc.sld, Y, ldy, N, nc, Pi, T);
        ABC_HIP(ctx, hipGetLastError());
        src.T = T;
    }

    const AjPlan pl = aj_plan(K, nc, Pi);
    const size_t bb = aj_batch(K, A, P, B);
    const size_t blk = (size_t)(1 + nc) * (1 + nc + P);
    double* part = (double*)abc_ws_alloc(ctx, bb * pl.nch * blk * 8);
    if (!part) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets_adjust: workspace exhausted");
    const int D = 1 + nc + Pi;
    const size_t lds_m = (size_t)(((D + 1) & ~1) + ((pl.TR + 1) & ~1) + pl.TR * aj_stride(nc, Pi)) * 8;
    const size_t lds_s = aj_solve_lds(nc);
    ABC_HIP(ctx, hipFuncSetAttribute((const void*)k_adj_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_s));
    for (size_t b0 = 0; b0 < B; b0 += bb) {
        const size_t nb = (B - b0 < bb) ? B - b0 : bb;
        hipLaunchKernelGGL(k_adj_moments, dim3((unsigned)pl.nch, (unsigned)nb), dim3(256), lds_m, ctx->stream, src, (const uint64_t*)idx,
                           (const double*)d, K, nc, Pi, kernel, pl.CH, pl.TR, b0, part);
        hipLaunchKernelGGL(k_adj_solve, dim3((unsigned)nb), dim3(256), lds_s, ctx->stream, src, (const uint64_t*)idx, (const double*)d, K,
                           nc, Pi, (int)A, kernel, sc.O, sc.KCO, (const double*)part, (int)pl.nch, b0, coef, out->rank, out->status);
        ABC_HIP(ctx, hipGetLastError());
    }

    if (keep) {
        keep->src = src;
        keep->O = sc.O;
        keep->KCO = sc.KCO;
        keep->nc = nc;
        keep->coef = coef;
        keep->dist = d;
    }
    if (out->theta || out->weight) {
        const int Wv = nc + Pi;
        int TR = Wv > 0 ? AJ_APPLY_DBL / Wv : 64;
        if (TR > 64) TR = 64;
        if (TR < 1) TR = 1;
        const int beta_lds = (nc * Pi <= AJ_APPLY_DBL) ? 1 : 0;
        const size_t lds_a = (size_t)((((size_t)TR * Wv + 1) & ~(size_t)1) + (beta_lds ? (size_t)nc * Pi : 0)) * 8;     // <= 64 KiB
        ABC_HIP(ctx, hipFuncSetAttribute((const void*)k_adj_apply, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
        const size_t tiles = (K + TR - 1) / TR;
        for (size_t b0 = 0; b0 < B; b0 += AJ_MAX_GRID_Y) {
            const size_t nb = (B - b0 < AJ_MAX_GRID_Y) ? B - b0 : AJ_MAX_GRID_Y;
            hipLaunchKernelGGL(k_adj_apply, dim3((unsigned)tiles, (unsigned)nb), dim3(256), lds_a, ctx->stream, src, (const uint64_t*)idx,
                               (const double*)d, K, nc, Pi, (int)A, kernel, sc.O, sc.KCO, (const double*)coef, TR, beta_lds, b0,
                               out->theta, out->weight);
            ABC_HIP(ctx, hipGetLastError());
        }
    }
    return ABC_OK;
}

static_assert(AJ_MAXA == 64 && AJ_MAXP == 1024, "limits of abc_rank_targets_adjust_dev (api.hip checks them)");
