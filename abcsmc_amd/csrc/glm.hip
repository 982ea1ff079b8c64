// ABC-GLM posterior of retained samples (abc_glm_rank_targets_dev, abc_glm_weighted_dev; the definition is in the header).
//
// A target's retained rows are gathered once into a row-major table Z[e][x(n) | theta(P)] with the adjustment's own reader
// (aj_val of adjust_dev.h), rows of weight <= 0 as zeros of weight 0, so that nothing below tells them from no row at all.
// Then, per batch of targets (a target's blocks never see another target):
//   k_glm_sums     grid (row chunks, targets): W, S2 and the sums of w z of a chunk; a thread owns (column, row mod 4) and runs one
//                  fma chain over its rows ascending, the four parts are added in order
//   k_glm_moments  grid (row chunks, targets): the means from the chunks' sums in chunk order (every block the same bits), the
//                  chunk's rows centred in LDS in tiles of 32, a thread owns a 4 x 4 block of the (n + P)^2 moments and runs one
//                  chain per entry over the chunk's rows; the chunk's block goes to the workspace (no atomics)
//   k_glm_solve    one work-group per target: the blocks summed in chunk order (the lower triangle, mirrored), the Cholesky
//                  factors of M_thth, Sigma_s, Q and S in LDS, C, c0, Sigma_s, T, u; the target's record for the kernels below
//   k_glm_peaks    one row per lane: v_e, t_e and log c_e (T in LDS, every lane reads the same entry); t_e goes to the workspace
//                  by parameter, [j][e], which is how the density reads it
//   k_glm_evid     one row per lane: r = (o - xbar) - C (theta_e - thbar), the triangular solve with the factor of S, log w_e - q / 2
//   k_glm_weights  one work-group per target: the two maxima, the two sums of exponentials, c^_e, ess, log_md
//   k_glm_stats    one work-group per (target, parameter): mean, var, the smallest and largest peak, lo_x, step, the density's constants
//   k_glm_dens     the hot path, k_dn_dens's structure (density.hip): work-groups over (target, parameter, chunk of GL_GC grid
//                  points), GL_R grid points per thread, (t_e[j], c^_e) staged in LDS in tiles, every lane reads the same entry, one
//                  fma chain per grid point over e ascending; the term is dn_kern (density_dev.h: fp64 argument, 2^r split)
//   k_glm_mode     the chunks' candidates in chunk order (G > GL_GC)
// and, for the *_summary entries only (abc_glm_rank_targets_summary_dev and its kin; the four older entries launch none of them):
//   k_glm_cdf      one work-group per (target, parameter): F_j(truth), a thread's fma chain over e = t (mod 256) of c^_e erfc(.),
//                  then the fixed tree
//   k_glm_quant    work-groups over (target, parameter, group of GL_QL levels): the root of F_j(x) = q for every level of the group
//                  in lockstep, a safeguarded Newton iteration (with Halley's correction) inside the guaranteed bracket
//                  [t_min + sigma z_q, t_max + sigma z_q]; one iteration is one pass over K, every thread summing its own entries
//                  e = t (mod 256) of c^_e erfc(.), c^_e exp(.) and c^_e a_e exp(.) for every level, a fixed shuffle tree per wave and
//                  the four waves' sums in order
// Chunk sizes depend on K only and tile sizes on nothing, every sum is a fixed chain or a fixed tree, and there are no floating-
// point atomics: a target's outputs are the same bits alone and in any batch, and whatever outputs are asked for.
// The bandwidths h_j are the marginal density's (launch_density_segs: bw.nrd0 on the weighted sample, or the given ones).
#include <math.h>

#include "abc_internal.h"
#include "adjust_dev.h"
#include "density_dev.h"

namespace {

constexpr int GL_MAX = 32;                                  // parameters and components at most
constexpr int GL_LD = GL_MAX + 1;                           // row stride of the 32 x 32 LDS matrices
constexpr int GL_D = 2 * GL_MAX;                            // columns of Z at most
constexpr int GL_MT = 32;                                   // rows of a k_glm_moments tile
constexpr int GL_PB = 128;                                  // rows of a k_glm_peaks work-group
constexpr int GL_EB = 64;                                   // rows of a k_glm_evid work-group
constexpr int GL_BS = 256;                                  // threads of the density's work-groups
constexpr int GL_R = 2;                                     // grid points per thread
constexpr int GL_GC = GL_BS * GL_R;                         // grid points per work-group
constexpr int GL_TILE = 1024;                               // entries staged in LDS at a time
constexpr size_t GL_BATCH_BYTES = (size_t)256 << 20;        // workspace of one batch of targets
constexpr unsigned GL_MAX_GRID_Y = 65535;
constexpr int GL_QL = 8;                                    // levels of a k_glm_quant work-group
constexpr int GL_QSLACK = 24;                               // steps of a level that may fail to halve its bracket
constexpr int GL_QCAP = 64 + GL_QSLACK + 2;                 // iterations at most (see k_glm_quant)
constexpr double GL_PIVOT = 1e-10;

// a target's record, made by k_glm_solve (doubles; matrices at row stride GL_MAX)
constexpr int GR_T = 0;                                     // T
constexpr int GR_C = GR_T + GL_MAX * GL_MAX;                // C, n x P
constexpr int GR_LS = GR_C + GL_MAX * GL_MAX;               // the Cholesky factor of S
constexpr int GR_U = GR_LS + GL_MAX * GL_MAX;               // u
constexpr int GR_TINV = GR_U + GL_MAX;                      // 1 / h_j^2
constexpr int GR_THB = GR_TINV + GL_MAX;                    // thbar
constexpr int GR_OBX = GR_THB + GL_MAX;                     // o - xbar
constexpr int GR_LDS = GR_OBX + GL_MAX;                     // log det S
constexpr int GR_W = GR_LDS + 1;                            // W
constexpr int GR_ST = GR_W + 1;                             // status bits (as a double)
constexpr int GR_LEN = GR_ST + 2;

struct GlSeg {                                              // per (target, parameter), made by k_glm_stats (all NaN: a bad target)
    double lo_x, step, den, c;                              // den = sqrt(2 pi T_jj), c = sqrt(log2(e) / 2) / sqrt(T_jj)
};

struct GlQs {                                               // per (target, parameter), made by k_glm_stats for the summaries
    double tlo, thi, mean, sd;                              // the smallest and largest peak of the counted rows, mean and sqrt(var)
};

struct GlLev {                                              // the levels of a summary (a kernel argument)
    double q[64], z[64];                                    // z = Phi^-1(q), from the host
    int nq;
};

struct GlSum {                                              // the caller's abc_summary, device pointers
    const double* truth;
    double *quant, *cdf;
};

struct GlSrc {
    AjSrc src;                  // scores S[i + sld k], parameters Y[i + ldy j]
    const uint64_t* idx;        // B x K rows (NULL: row e itself)
    const double* om;           // weight of row i (NULL: none)
    const double* w;            // weight of entry e (NULL: none); one of om and w at most
    const double* O;            // the observed scores, O[b KCO + k]
    int KCO;
};

struct GlOut {
    int G;
    double cut;
    double *dens, *lo_x, *step, *mode, *mode_dens, *mean, *var, *ess, *log_md, *C, *c0, *sigma_s, *T, *peaks, *c;
    int32_t* status;
};

struct GlWs {                   // one batch's blocks; b below is the target's place in the batch
    double* Z;                  // [b][e][D]
    double* wv;                 // [b][e]
    double* part1;              // [b][chunk][D + 3]
    double* part2;              // [b][chunk][D][D]
    double* rec;                // [b][GR_LEN]
    double* tpk;                // [b][j][e]
    double* logc;               // [b][e]
    double* logn;               // [b][e]
    double* chat;               // [b][e]
    GlSeg* seg;                 // [b][j]
    double* pf;                 // [b][j][chunk of the grid]
    int* pg;
    GlQs* qs;                   // [b][j]; NULL without a summary
};

typedef AjChunks GlPlan;        // the adjustment's chunks of a target's rows (adjust_dev.h): from K alone
inline GlPlan gl_plan(size_t K) { return aj_chunks(K); }

// grid (tiles of 64 rows, targets of the batch)
__global__ __launch_bounds__(256) void k_glm_gather(GlSrc g, size_t K, int n, int P, size_t b0, GlWs ws) {
    __shared__ double sw[64];
    __shared__ size_t si[64];
    const int t = threadIdx.x, D = n + P;
    const size_t bl = blockIdx.y, b = b0 + bl, e0 = (size_t)blockIdx.x * 64;
    const int nr = (K - e0 < 64) ? (int)(K - e0) : 64;
    if (t < nr) {
        const size_t e = e0 + t, i = g.idx ? (size_t)g.idx[b * K + e] : e;
        const double w = g.om ? g.om[i] : (g.w ? g.w[e] : 1.0);
        sw[t] = w > 0.0 ? w : 0.0;
        si[t] = i;
        ws.wv[bl * K + e] = sw[t];
    }
    __syncthreads();
    double* z = ws.Z + (bl * K + e0) * (size_t)D;
    for (int q = t; q < nr * D; q += 256) {
        const int r = q / D, c = q % D;
        z[q] = sw[r] > 0.0 ? aj_val(g.src, si[r], c, n) : 0.0;
    }
}

// grid (row chunks, targets of the batch)
__global__ __launch_bounds__(256) void k_glm_sums(size_t K, int D, size_t CH, GlWs ws) {
    __shared__ double red[4][GL_D], rw[4], rs[4];
    __shared__ int bad;
    const int t = threadIdx.x, c = t & 63, part = t >> 6;
    const size_t bl = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
    const size_t e0 = ch * CH, e1 = (e0 + CH < K) ? e0 + CH : K;
    const double* z = ws.Z + bl * K * (size_t)D;
    const double* wv = ws.wv + bl * K;
    if (t == 0) bad = 0;
    __syncthreads();
    double s = 0.0, W = 0.0, S2 = 0.0;
    int nf = 0;
    for (size_t e = e0 + part; e < e1; e += 4) {
        const double w = wv[e];
        W += w;
        S2 = fma(w, w, S2);
        if (c < D) {
            const double v = z[e * D + c];
            if (!isfinite(v)) nf = 1;
            s = fma(w, v, s);
        }
    }
    if (nf) atomicOr(&bad, 1);
    if (c < D) red[part][c] = s;
    if (c == 0) { rw[part] = W; rs[part] = S2; }
    __syncthreads();
    double* o = ws.part1 + (bl * nch + ch) * (size_t)(D + 3);
    if (t < D) o[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (t == 0) {
        o[D] = ((rw[0] + rw[1]) + rw[2]) + rw[3];
        o[D + 1] = ((rs[0] + rs[1]) + rs[2]) + rs[3];
        o[D + 2] = bad ? 1.0 : 0.0;
    }
}

// grid (row chunks, targets of the batch)
__global__ __launch_bounds__(256) void k_glm_moments(size_t K, int D, size_t CH, GlWs ws) {
    __shared__ double tile[GL_MT][GL_D + 1], mean[GL_D], sw[GL_MT];
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const size_t bl = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
    const size_t e0 = ch * CH, e1 = (e0 + CH < K) ? e0 + CH : K;
    const double* z = ws.Z + bl * K * (size_t)D;
    const double* wv = ws.wv + bl * K;
    const double* p1 = ws.part1 + bl * nch * (size_t)(D + 3);
    if (t < GL_D) {
        double s = 0.0, W = 0.0;
        if (t < D)
            for (size_t q = 0; q < nch; q++) {
                s += p1[q * (D + 3) + t];
                W += p1[q * (D + 3) + D];
            }
        mean[t] = t < D ? s / W : 0.0;
    }
    for (int q = t; q < GL_MT * (GL_D + 1); q += 256) (&tile[0][0])[q] = 0.0;
    __syncthreads();
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
    for (size_t base = e0; base < e1; base += GL_MT) {
        const int nr = (e1 - base < (size_t)GL_MT) ? (int)(e1 - base) : GL_MT;
        for (int q = t; q < nr * D; q += 256) {
            const int r = q / D, c = q % D;
            tile[r][c] = z[base * D + q] - mean[c];
        }
        if (t < nr) sw[t] = wv[base + t];
        __syncthreads();
        for (int r = 0; r < nr; r++) {
            const double w = sw[r];
            double u[4], v[4];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                u[a] = w * tile[r][4 * ti + a];
                v[a] = tile[r][4 * tj + a];
            }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] = fma(u[a], v[b], acc[a][b]);
        }
        __syncthreads();
    }
    double* o = ws.part2 + (bl * nch + ch) * (size_t)D * D;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int r = 4 * ti + a, c = 4 * tj + b;
            if (r < D && c <= r) o[r * D + c] = acc[a][b];
        }
}

// ---- the small dense pieces of k_glm_solve: m x m matrices in LDS at row stride GL_LD, all 256 threads enter ----
// in place, the lower triangle: A = L L'.  A pivot <= rel times its own diagonal entry (or NaN) sets *flag (flag NULL: no check)
__device__ void gl_chol(double* A, int m, double rel, int* flag) {
    const int t = threadIdx.x;
    for (int j = 0; j < m; j++) {
        __syncthreads();
        if (t == 0) {
            const double a = A[j * GL_LD + j];
            double d = a;
            for (int k = 0; k < j; k++) d = fma(-A[j * GL_LD + k], A[j * GL_LD + k], d);
            if (flag && !(d > rel * a)) *flag = 1;
            A[j * GL_LD + j] = sqrt(d);
        }
        __syncthreads();
        if (t > j && t < m) {
            double s = A[t * GL_LD + j];
            for (int k = 0; k < j; k++) s = fma(-A[t * GL_LD + k], A[j * GL_LD + k], s);
            A[t * GL_LD + j] = s / A[j * GL_LD + j];
        }
    }
    __syncthreads();
}
// L X = B in place, B m x r at row stride GL_LD; one column per thread
__device__ void gl_fwd(const double* L, int m, double* B, int r) {
    const int t = threadIdx.x;
    if (t < r)
        for (int i = 0; i < m; i++) {
            double s = B[i * GL_LD + t];
            for (int k = 0; k < i; k++) s = fma(-L[i * GL_LD + k], B[k * GL_LD + t], s);
            B[i * GL_LD + t] = s / L[i * GL_LD + i];
        }
    __syncthreads();
}
// L' X = B in place
__device__ void gl_bwd(const double* L, int m, double* B, int r) {
    const int t = threadIdx.x;
    if (t < r)
        for (int i = m - 1; i >= 0; i--) {
            double s = B[i * GL_LD + t];
            for (int k = m - 1; k > i; k--) s = fma(-L[k * GL_LD + i], B[k * GL_LD + t], s);
            B[i * GL_LD + t] = s / L[i * GL_LD + i];
        }
    __syncthreads();
}

// one work-group per target of the batch; hseg: the bandwidths' records of all targets, [b][j]
__global__ __launch_bounds__(256) void k_glm_solve(size_t K, int n, int P, size_t nch, size_t b0, GlSrc g, const DnSeg* __restrict__ hseg,
                                                   GlOut o, GlWs ws) {
    extern __shared__ double lds[];
    double* M = lds;                                        // D x D at row stride GL_D + 1: x first, then theta
    double* Lt = M + GL_D * (GL_D + 1);                     // the factor of M_thth
    double* Ct = Lt + GL_MAX * GL_LD;                       // M_thth^-1 M_thx, P x n
    double* Sg = Ct + GL_MAX * GL_LD;                       // Sigma_s, then its factor
    double* Bm = Sg + GL_MAX * GL_LD;                       // Ls^-1 C, n x P
    double* Qm = Bm + GL_MAX * GL_LD;                       // Q, then its factor
    double* Tm = Qm + GL_MAX * GL_LD;                       // T
    double* Sm = Tm + GL_MAX * GL_LD;                       // S, then its factor
    double* mean = Sm + GL_MAX * GL_LD;                     // GL_D
    double* vec = mean + GL_D;                              // column 0 of a GL_LD-strided block: o - xbar, then Ls^-1 of it
    double* tinv = vec + GL_MAX * GL_LD;                    // GL_MAX
    double* uu = tinv + GL_MAX;                             // GL_MAX
    __shared__ int f0, f1, fn, fh;
    __shared__ double sW, sS2, sbad;
    const int t = threadIdx.x, D = n + P, MS = GL_D + 1;
    const size_t bl = blockIdx.x, b = b0 + bl;
    const double* p1 = ws.part1 + bl * nch * (size_t)(D + 3);
    const double* p2 = ws.part2 + bl * nch * (size_t)D * D;
    if (t == 0) { f0 = 0; f1 = 0; fn = 0; fh = 0; }
    if (t < D + 3) {
        double s = 0.0;
        for (size_t q = 0; q < nch; q++) s += p1[q * (D + 3) + t];
        if (t < D) mean[t] = s;
        else if (t == D) sW = s;
        else if (t == D + 1) sS2 = s;
        else sbad = s;
    }
    __syncthreads();
    const double W = sW, neff = W * W / sS2;
    if (t < D) mean[t] /= W;
    for (int q = t; q < D * D; q += 256) {
        const int r = q / D, c = q % D;
        if (c <= r) {
            double s = 0.0;
            for (size_t k = 0; k < nch; k++) s += p2[k * (size_t)D * D + q];
            s /= W;
            M[r * MS + c] = s;
            M[c * MS + r] = s;
        }
    }
    __syncthreads();
    // M_thth = L L', C' = M_thth^-1 M_thx
    for (int q = t; q < P * P; q += 256) Lt[(q / P) * GL_LD + q % P] = M[(n + q / P) * MS + n + q % P];
    for (int q = t; q < P * n; q += 256) Ct[(q / n) * GL_LD + q % n] = M[(n + q / n) * MS + q % n];
    gl_chol(Lt, P, GL_PIVOT, &f0);
    gl_fwd(Lt, P, Ct, n);
    gl_bwd(Lt, P, Ct, n);
    // Sigma_s = (M_xx - M_xth C') n_eff / (n_eff - P - 1), the lower triangle mirrored; o - xbar
    const double fs = neff / (neff - (double)(P + 1));
    for (int q = t; q < n * n; q += 256) {
        const int k = q / n, l = q % n;
        if (l <= k) {
            double s = M[k * MS + l];
            for (int j = 0; j < P; j++) s = fma(-M[(n + j) * MS + k], Ct[j * GL_LD + l], s);
            s *= fs;
            Sg[k * GL_LD + l] = s;
            Sg[l * GL_LD + k] = s;
        }
    }
    if (t < n) vec[t * GL_LD] = g.O[b * (size_t)g.KCO + t] - mean[t];
    if (t < P) {
        const double h = hseg[b * P + t].h;
        tinv[t] = 1.0 / (h * h);
        if (!isfinite(h)) atomicOr(&fh, 1);                    // (the rule reads every entry of the column, uncounted ones too)
    }
    if (t == 0 && !(neff > (double)(P + 1))) fn = 1;
    __syncthreads();
    double* rec = ws.rec + bl * GR_LEN;
    if (t < n) rec[GR_OBX + t] = vec[t * GL_LD];
    if (o.sigma_s)
        for (int q = t; q < n * n; q += 256) o.sigma_s[b * (size_t)n * n + q] = Sg[(q / n) * GL_LD + q % n];
    // S = Sigma_s + C Sigma_theta C' before Sigma_s is factored
    for (int q = t; q < n * n; q += 256) {
        const int k = q / n, l = q % n;
        if (l <= k) {
            double s = Sg[k * GL_LD + l];
            for (int j = 0; j < P; j++) s = fma(Ct[j * GL_LD + k] / tinv[j], Ct[j * GL_LD + l], s);
            Sm[k * GL_LD + l] = s;
            Sm[l * GL_LD + k] = s;
        }
    }
    for (int q = t; q < n * P; q += 256) Bm[(q / P) * GL_LD + q % P] = Ct[(q % P) * GL_LD + q / P];
    gl_chol(Sg, n, GL_PIVOT, &f1);
    gl_fwd(Sg, n, Bm, P);
    gl_fwd(Sg, n, vec, 1);
    // Q = C' Sigma_s^-1 C + Sigma_theta^-1, u = C' Sigma_s^-1 (o - xbar), T = Q^-1
    for (int q = t; q < P * P; q += 256) {
        const int i = q / P, j = q % P;
        if (j <= i) {
            double s = i == j ? tinv[i] : 0.0;
            for (int k = 0; k < n; k++) s = fma(Bm[k * GL_LD + i], Bm[k * GL_LD + j], s);
            Qm[i * GL_LD + j] = s;
            Qm[j * GL_LD + i] = s;
        }
        Tm[i * GL_LD + j] = i == j ? 1.0 : 0.0;
    }
    if (t < P) {
        double s = 0.0;
        for (int k = 0; k < n; k++) s = fma(Bm[k * GL_LD + t], vec[k * GL_LD], s);
        uu[t] = s;
    }
    gl_chol(Qm, P, 0.0, nullptr);                              // (positive definite by construction: Sigma_theta^-1 > 0 on its diagonal)
    gl_fwd(Qm, P, Tm, P);
    gl_bwd(Qm, P, Tm, P);
    gl_chol(Sm, n, 0.0, nullptr);                              // (Sigma_s, whose pivots have passed, plus a positive semi-definite term)
    // one bit, the first that applies: non-finite input, n_eff (no counted row gives NaN moments, and is this bit), the pivots of
    // M_thth, a non-finite bandwidth (from an uncounted row: the rule reads every entry), the pivots of Sigma_s; what follows a
    // failed step is computed from NaNs
    const int st = sbad != 0.0 ? 4 : (fn ? 2 : (f0 ? 1 : (fh ? 4 : (f1 ? 2 : 0))));
    const double nan = dn_nan();
    // the record and the model outputs: T's lower triangle mirrored
    for (int q = t; q < P * P; q += 256) {
        const int i = q / P, j = q % P;
        const double v = j <= i ? Tm[i * GL_LD + j] : Tm[j * GL_LD + i];
        rec[GR_T + i * GL_MAX + j] = v;
        if (o.T) o.T[b * (size_t)P * P + q] = st ? nan : v;
    }
    for (int q = t; q < n * P; q += 256) {
        const int k = q / P, j = q % P;
        const double v = Ct[j * GL_LD + k];
        rec[GR_C + k * GL_MAX + j] = v;
        if (o.C) o.C[b * (size_t)n * P + q] = st ? nan : v;
    }
    for (int q = t; q < n * n; q += 256) rec[GR_LS + (q / n) * GL_MAX + q % n] = Sm[(q / n) * GL_LD + q % n];
    if (t < P) {
        rec[GR_U + t] = uu[t];
        rec[GR_TINV + t] = tinv[t];
        rec[GR_THB + t] = mean[n + t];
    }
    if (t < n && o.c0) {
        double s = mean[t];
        for (int j = 0; j < P; j++) s = fma(-Ct[j * GL_LD + t], mean[n + j], s);
        o.c0[b * (size_t)n + t] = st ? nan : s;
    }
    if (st && o.sigma_s)
        for (int q = t; q < n * n; q += 256) o.sigma_s[b * (size_t)n * n + q] = nan;
    if (t == 0) {
        double ld = 0.0;
        for (int k = 0; k < n; k++) ld += log(Sm[k * GL_LD + k]);
        rec[GR_LDS] = 2.0 * ld;
        rec[GR_W] = W;
        rec[GR_ST] = (double)st;
        if (o.status) o.status[b] = st;
    }
}

constexpr size_t GL_SOLVE_LDS = (size_t)(GL_D * (GL_D + 1) + 8 * GL_MAX * GL_LD + GL_D + 2 * GL_MAX) * 8;

// grid (tiles of GL_PB rows, targets of the batch)
__global__ __launch_bounds__(GL_PB) void k_glm_peaks(size_t K, int n, int P, size_t b0, GlOut o, GlWs ws) {
    __shared__ double vr[GL_PB][GL_LD], Tl[GL_MAX][GL_LD], u[GL_MAX], tinv[GL_MAX], thb[GL_MAX];
    const int t = threadIdx.x, D = n + P;
    const size_t bl = blockIdx.y, b = b0 + bl, e0 = (size_t)blockIdx.x * GL_PB;
    const int nr = (K - e0 < (size_t)GL_PB) ? (int)(K - e0) : GL_PB;
    const double* rec = ws.rec + bl * GR_LEN;
    for (int q = t; q < P * P; q += GL_PB) Tl[q / P][q % P] = rec[GR_T + (q / P) * GL_MAX + q % P];
    if (t < P) {
        u[t] = rec[GR_U + t];
        tinv[t] = rec[GR_TINV + t];
        thb[t] = rec[GR_THB + t];
    }
    __syncthreads();
    const double* z = ws.Z + (bl * K + e0) * (size_t)D;
    for (int q = t; q < nr * P; q += GL_PB) {
        const int r = q / P, j = q % P;
        vr[r][j] = z[r * D + n + j] - thb[j];
    }
    __syncthreads();
    if (t >= nr) return;
    const size_t e = e0 + t;
    const bool bad = rec[GR_ST] != 0.0, counted = ws.wv[bl * K + e] > 0.0;
    double q1 = 0.0;
    for (int j = 0; j < P; j++) {
        const double d = vr[t][j];
        q1 = fma(d * d, tinv[j], q1);
        vr[t][j] = fma(tinv[j], d, u[j]);
    }
    double q2 = 0.0;
    for (int j = 0; j < P; j++) {
        double s = 0.0;
        for (int k = 0; k < P; k++) s = fma(Tl[j][k], vr[t][k], s);
        q2 = fma(vr[t][j], s, q2);
        const double tj = bad ? dn_nan() : thb[j] + s;
        ws.tpk[(bl * P + j) * K + e] = tj;
        if (o.peaks) o.peaks[(b * K + e) * P + j] = counted ? tj : dn_nan();      // (an uncounted row has no peak)
    }
    ws.logc[bl * K + e] = log(ws.wv[bl * K + e]) - 0.5 * (q1 - q2);
}

// grid (tiles of GL_EB rows, targets of the batch)
__global__ __launch_bounds__(GL_EB) void k_glm_evid(size_t K, int n, int P, GlWs ws) {
    __shared__ double dr[GL_EB][GL_LD], yr[GL_EB][GL_LD], Cl[GL_MAX][GL_LD], Ls[GL_MAX][GL_LD], obx[GL_MAX], thb[GL_MAX];
    const int t = threadIdx.x, D = n + P;
    const size_t bl = blockIdx.y, e0 = (size_t)blockIdx.x * GL_EB;
    const int nr = (K - e0 < (size_t)GL_EB) ? (int)(K - e0) : GL_EB;
    const double* rec = ws.rec + bl * GR_LEN;
    for (int q = t; q < n * P; q += GL_EB) Cl[q / P][q % P] = rec[GR_C + (q / P) * GL_MAX + q % P];
    for (int q = t; q < n * n; q += GL_EB) Ls[q / n][q % n] = rec[GR_LS + (q / n) * GL_MAX + q % n];
    if (t < n) obx[t] = rec[GR_OBX + t];
    if (t < P) thb[t] = rec[GR_THB + t];
    __syncthreads();
    const double* z = ws.Z + (bl * K + e0) * (size_t)D;
    for (int q = t; q < nr * P; q += GL_EB) {
        const int r = q / P, j = q % P;
        dr[r][j] = z[r * D + n + j] - thb[j];
    }
    __syncthreads();
    if (t >= nr) return;
    double qq = 0.0;
    for (int k = 0; k < n; k++) {
        double s = obx[k];
        for (int j = 0; j < P; j++) s = fma(-Cl[k][j], dr[t][j], s);
        for (int l = 0; l < k; l++) s = fma(-Ls[k][l], yr[t][l], s);
        const double y = s / Ls[k][k];
        yr[t][k] = y;
        qq = fma(y, y, qq);
    }
    ws.logn[bl * K + e0 + t] = log(ws.wv[bl * K + e0 + t]) - 0.5 * qq;
}

// a fixed tree over the 256 threads of a work-group
__device__ __forceinline__ double gl_tree_sum(double v, double* r) {
    const int t = threadIdx.x;
    __syncthreads();
    r[t] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) r[t] += r[t + st];
        __syncthreads();
    }
    return r[0];
}
__device__ __forceinline__ double gl_tree_max(double v, double* r) {
    const int t = threadIdx.x;
    __syncthreads();
    r[t] = v;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) r[t] = fmax(r[t], r[t + st]);
        __syncthreads();
    }
    return r[0];
}

// one work-group per target of the batch
__global__ __launch_bounds__(256) void k_glm_weights(size_t K, int n, size_t b0, GlOut o, GlWs ws) {
    __shared__ double r[256];
    const int t = threadIdx.x;
    const size_t bl = blockIdx.x, b = b0 + bl;
    const double* rec = ws.rec + bl * GR_LEN;
    const double* lc = ws.logc + bl * K;
    const double* ln = ws.logn + bl * K;
    const bool bad = rec[GR_ST] != 0.0;
    const double ninf = -INFINITY;
    double m1 = ninf, m2 = ninf;
    for (size_t e = t; e < K; e += 256) {
        m1 = fmax(m1, lc[e]);
        m2 = fmax(m2, ln[e]);
    }
    m1 = gl_tree_max(m1, r);
    m2 = gl_tree_max(m2, r);
    double s1 = 0.0, s2 = 0.0;
    for (size_t e = t; e < K; e += 256) {
        s1 += exp(lc[e] - m1);
        s2 += exp(ln[e] - m2);
    }
    s1 = gl_tree_sum(s1, r);
    s2 = gl_tree_sum(s2, r);
    double q = 0.0;
    for (size_t e = t; e < K; e += 256) {
        const double c = bad ? dn_nan() : exp(lc[e] - m1) / s1;
        ws.chat[bl * K + e] = c;
        if (o.c) o.c[b * K + e] = c;
        q = fma(c, c, q);
    }
    q = gl_tree_sum(q, r);
    if (t != 0) return;
    if (o.ess) o.ess[b] = bad ? dn_nan() : 1.0 / q;
    if (o.log_md)
        o.log_md[b] = bad ? dn_nan() : (m2 + log(s2)) - 0.5 * ((double)n * 1.8378770664093453 + rec[GR_LDS]) - log(rec[GR_W]);
}

// grid (P, targets of the batch)
__global__ __launch_bounds__(256) void k_glm_stats(size_t K, int P, size_t b0, GlOut o, GlWs ws) {
    __shared__ double r[256];
    const int t = threadIdx.x, j = (int)blockIdx.x;
    const size_t bl = blockIdx.y, b = b0 + bl, sg = b * P + j;
    const double* rec = ws.rec + bl * GR_LEN;
    const double* tp = ws.tpk + (bl * P + j) * K;
    const double* ch = ws.chat + bl * K;
    const double* wv = ws.wv + bl * K;
    const bool bad = rec[GR_ST] != 0.0;
    const double Tjj = rec[GR_T + j * GL_MAX + j];
    double m = 0.0, lo = INFINITY, hi = -INFINITY;
    for (size_t e = t; e < K; e += 256) {
        m = fma(ch[e], tp[e], m);
        if (wv[e] > 0.0) {
            lo = fmin(lo, tp[e]);
            hi = fmax(hi, tp[e]);
        }
    }
    m = gl_tree_sum(m, r);
    lo = -gl_tree_max(-lo, r);
    hi = gl_tree_max(hi, r);
    double v = 0.0;
    for (size_t e = t; e < K; e += 256) {
        const double d = tp[e] - m;
        v = fma(ch[e], d * d, v);
    }
    v = gl_tree_sum(v, r);
    if (t != 0) return;
    GlSeg p;
    p.lo_x = p.step = p.den = p.c = dn_nan();
    if (!bad) {
        const double sd = sqrt(Tjj);
        p.lo_x = lo - o.cut * sd;
        p.step = ((hi + o.cut * sd) - p.lo_x) / (double)(o.G - 1);
        p.den = sd * 2.5066282746310002;                       // sqrt(2 pi)
        p.c = 0.8493218002880191 / sd;                         // sqrt(log2(e) / 2)
    }
    ws.seg[bl * P + j] = p;
    if (ws.qs) {
        GlQs s;
        s.tlo = lo; s.thi = hi; s.mean = m; s.sd = sqrt(Tjj + v);
        ws.qs[bl * P + j] = s;
    }
    if (o.mean) o.mean[sg] = bad ? dn_nan() : m;
    if (o.var) o.var[sg] = bad ? dn_nan() : Tjj + v;
    if (o.lo_x) o.lo_x[sg] = p.lo_x;
    if (o.step) o.step[sg] = p.step;
}

// grid (P x nchunk, targets of the batch)
__global__ __launch_bounds__(GL_BS) void k_glm_dens(size_t K, int P, size_t b0, int nchunk, GlOut o, GlWs ws) {
    __shared__ __attribute__((aligned(16))) double2 tile[GL_TILE];
    __shared__ double rf[GL_BS];
    __shared__ int rg[GL_BS];
    const int t = threadIdx.x, j = (int)(blockIdx.x % (unsigned)P), c = (int)(blockIdx.x / (unsigned)P), G = o.G;
    const size_t bl = blockIdx.y, b = b0 + bl, sg = b * P + j;
    const GlSeg p = ws.seg[bl * P + j];
    const bool bad = isnan(p.den);
    const double* tp = ws.tpk + (bl * P + j) * K;
    const double* ch = ws.chat + bl * K;
    double x[GL_R], acc[GL_R];
#pragma unroll
    for (int r = 0; r < GL_R; r++) {
        x[r] = fma((double)(c * GL_GC + r * GL_BS + t), p.step, p.lo_x);
        acc[r] = 0.0;
    }
    if (!bad)
        for (size_t base = 0; base < K; base += GL_TILE) {
            const int len = (K - base < (size_t)GL_TILE) ? (int)(K - base) : GL_TILE;
            for (int i = t; i < len; i += GL_BS) tile[i] = make_double2(tp[base + i], ch[base + i]);
            __syncthreads();
#pragma unroll 4
            for (int i = 0; i < len; i++) {
                const double2 vw = tile[i];
#pragma unroll
                for (int r = 0; r < GL_R; r++) acc[r] = fma(vw.y, dn_kern((x[r] - vw.x) * p.c), acc[r]);
            }
            __syncthreads();
        }
    double bf = -1.0;
    int bg = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < GL_R; r++) {                           // g ascending in r: a tie keeps the smaller g
        const int g = c * GL_GC + r * GL_BS + t;
        const double f = bad ? dn_nan() : acc[r] / p.den;
        if (g < G) {
            if (o.dens) o.dens[sg * (size_t)G + g] = f;
            if (f > bf) { bf = f; bg = g; }
        }
    }
    if (!o.mode && !o.mode_dens) return;
    rf[t] = bf;
    rg[t] = bg;
    __syncthreads();
    for (int st = GL_BS / 2; st > 0; st >>= 1) {
        if (t < st) {
            const double f2 = rf[t + st];
            const int g2 = rg[t + st];
            if (f2 > rf[t] || (f2 == rf[t] && g2 < rg[t])) { rf[t] = f2; rg[t] = g2; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    if (nchunk > 1) {
        ws.pf[(bl * P + j) * nchunk + c] = rf[0];
        ws.pg[(bl * P + j) * nchunk + c] = rg[0];
        return;
    }
    const bool none = bad || rg[0] >= G;
    if (o.mode) o.mode[sg] = none ? dn_nan() : fma((double)rg[0], p.step, p.lo_x);
    if (o.mode_dens) o.mode_dens[sg] = none ? dn_nan() : rf[0];
}

// the chunks' candidates in chunk order (g ascending: a tie keeps the earlier chunk); one thread per (target, parameter) of the batch
__global__ __launch_bounds__(256) void k_glm_mode(size_t nseg, size_t sg0, int nchunk, GlOut o, GlWs ws) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    double bf = -1.0;
    int bg = 0x7fffffff;
    for (int c = 0; c < nchunk; c++) {
        const double f = ws.pf[s * nchunk + c];
        if (f > bf) { bf = f; bg = ws.pg[s * nchunk + c]; }
    }
    const GlSeg p = ws.seg[s];
    const bool none = isnan(p.den) || bg >= o.G;
    if (o.mode) o.mode[sg0 + s] = none ? dn_nan() : fma((double)bg, p.step, p.lo_x);
    if (o.mode_dens) o.mode_dens[sg0 + s] = none ? dn_nan() : bf;
}

// ---- the exact CDF and quantiles of the marginal mixture (the *_summary entries) ----
// F_j(x) = sum_e c^_e Phi((x - t_e[j]) / sigma) = sum_e c^_e erfc(a_e) / 2 with a_e = (t_e[j] - x) / (sigma sqrt 2).  An uncounted row
// has c^_e = 0 exactly and a finite t_e (its row of Z is zero), so its term is an exact zero and the sums run over every e.

// grid (P, targets of the batch)
__global__ __launch_bounds__(256) void k_glm_cdf(size_t K, int P, size_t b0, GlSum sm, GlWs ws) {
    __shared__ double r[256];
    const int t = threadIdx.x, j = (int)blockIdx.x;
    const size_t bl = blockIdx.y, sg = (b0 + bl) * P + j;
    const double* rec = ws.rec + bl * GR_LEN;
    const double* tp = ws.tpk + (bl * P + j) * K;
    const double* ch = ws.chat + bl * K;
    const double x = sm.truth[sg];
    const double ri = 1.0 / (sqrt(rec[GR_T + j * GL_MAX + j]) * 1.4142135623730951);
    double s = 0.0;
    for (size_t e = t; e < K; e += 256) s = fma(ch[e], erfc((tp[e] - x) * ri), s);
    s = gl_tree_sum(s, r);
    if (t != 0) return;
    double F = 0.5 * s;
    if (x == INFINITY) F = 1.0;
    if (x == -INFINITY) F = 0.0;
    sm.cdf[sg] = rec[GR_ST] != 0.0 ? dn_nan() : F;             // (a NaN truth: every term is NaN)
}

// the doubles in ascending order as unsigned integers (-0.0 right below +0.0), and back
__device__ __forceinline__ uint64_t gl_ord(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double gl_unord(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
// a fixed tree over the 64 lanes of a wave; lane 0 holds the sum
__device__ __forceinline__ double gl_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// grid (P x groups of GL_QL levels, targets of the batch).  Level l of the group belongs to thread l, which keeps its bracket
// (lo, hi), the values F found at its ends (NaN: not evaluated), the next point x and its allowance; the work-group reads x and
// the activity flags from LDS, and every thread sums its own entries for every active level.
// The bracket.  Every peak lies in [t_min, t_max], so Phi((x - t_max) / sigma) <= F(x) <= Phi((x - t_min) / sigma) and the root lies
// in [t_min + sigma z, t_max + sigma z]; the ends are widened by 2^-49 of their terms and four doubles for the rounding of z, sigma
// and the two operations.  They are not evaluated: an end moves only to a point the device has evaluated, F < q to lo, else to hi.
// A step.  s = r / f with r = F - q, Halley's correction s / (1 - s f' / (2 f)) where that factor is within [1/2, 2]; a point equal
// to x moves one double towards the root.  The point is taken if it lies strictly inside the bracket and the level's allowance is
// not spent; otherwise the next point is the middle of the bracket counted in doubles.
// The cap.  W = the doubles from lo to hi.  A step either leaves W' <= ceil(W / 2) (every middle point does) or it costs one of the
// GL_QSLACK allowances; W < 2^64, so after at most 64 + GL_QSLACK steps W <= 1: no double lies strictly inside.  GL_QCAP is that
// plus two.  The result is the end whose evaluated F is nearer q (hi on a tie; the evaluated one where only one is).
__global__ __launch_bounds__(256) void k_glm_quant(size_t K, int P, size_t b0, GlLev lv, GlSum sm, GlWs ws) {
    __shared__ double part[3][GL_QL][4], xs[GL_QL];
    __shared__ int act[GL_QL], nact;
    const int t = threadIdx.x, j = (int)(blockIdx.x % (unsigned)P), l0 = (int)(blockIdx.x / (unsigned)P) * GL_QL;
    const int nl = lv.nq - l0 < GL_QL ? lv.nq - l0 : GL_QL, lane = t & 63, wave = t >> 6;
    const size_t bl = blockIdx.y, b = b0 + bl;
    const double* rec = ws.rec + bl * GR_LEN;
    const double* tp = ws.tpk + (bl * P + j) * K;
    const double* ch = ws.chat + bl * K;
    double* out = sm.quant + (b * lv.nq + l0) * (size_t)P + j;       // level l at out[l P]
    if (rec[GR_ST] != 0.0) {
        if (t < nl) out[(size_t)t * P] = dn_nan();
        return;
    }
    const double sd = sqrt(rec[GR_T + j * GL_MAX + j]), ri = 1.0 / (sd * 1.4142135623730951);
    const double kf = ri * 0.5641895835477563, kd = 2.0 * ri;    // f = kf sum c exp(-a^2), f' / f = kd sum c a exp(-a^2) / sum c exp(-a^2)
    double q = 0.0, lo = 0.0, hi = 0.0, Flo = dn_nan(), Fhi = dn_nan(), x = 0.0;
    int slack = GL_QSLACK, it = 0;
    if (t < nl) {
        const GlQs s = ws.qs[bl * P + j];
        const double z = lv.z[l0 + t], sz = sd * z, eps = 1.7763568394002505e-15;      // 2^-49
        q = lv.q[l0 + t];
        lo = gl_unord(gl_ord((s.tlo + sz) - eps * (fabs(s.tlo) + fabs(sz))) - 4);
        hi = gl_unord(gl_ord((s.thi + sz) + eps * (fabs(s.thi) + fabs(sz))) + 4);
        x = fma(s.sd, z, s.mean);                                 // the quantile of a Gaussian of the mixture's mean and variance
        if (!(x > lo && x < hi)) x = gl_unord(gl_ord(lo) + (gl_ord(hi) - gl_ord(lo)) / 2);
        xs[t] = x;
        act[t] = 1;
    }
    if (t == 0) nact = nl;
    __syncthreads();
    while (nact > 0 && it < GL_QCAP) {                             // (uniform: nact is read between two barriers)
        double xl[GL_QL], a0[GL_QL], a1[GL_QL], a2[GL_QL];
        bool on[GL_QL];
#pragma unroll
        for (int l = 0; l < GL_QL; l++) {
            on[l] = l < nl && act[l] != 0;
            xl[l] = on[l] ? xs[l] : 0.0;
            a0[l] = a1[l] = a2[l] = 0.0;
        }
        for (size_t e = t; e < K; e += 256) {
            const double te = tp[e], ce = ch[e];
#pragma unroll
            for (int l = 0; l < GL_QL; l++)
                if (on[l]) {                                       // (uniform over the work-group)
                    const double a = (te - xl[l]) * ri, ex = ce * exp(-(a * a));
                    a0[l] = fma(ce, erfc(a), a0[l]);
                    a1[l] += ex;
                    a2[l] = fma(a, ex, a2[l]);
                }
        }
#pragma unroll
        for (int l = 0; l < GL_QL; l++)
            if (on[l]) {
                const double s0 = gl_wave_sum(a0[l]), s1 = gl_wave_sum(a1[l]), s2 = gl_wave_sum(a2[l]);
                if (lane == 0) { part[0][l][wave] = s0; part[1][l][wave] = s1; part[2][l][wave] = s2; }
            }
        __syncthreads();
        it++;
        if (t < nl && act[t]) {
            const double F = 0.5 * (((part[0][t][0] + part[0][t][1]) + part[0][t][2]) + part[0][t][3]);
            const double E = ((part[1][t][0] + part[1][t][1]) + part[1][t][2]) + part[1][t][3];
            const double A = ((part[2][t][0] + part[2][t][1]) + part[2][t][2]) + part[2][t][3];
            const double r = F - q;
            const uint64_t W = gl_ord(hi) - gl_ord(lo);
            if (r < 0.0) { lo = x; Flo = F; } else { hi = x; Fhi = F; }
            const uint64_t W2 = gl_ord(hi) - gl_ord(lo);
            if (W2 <= 1) {
                act[t] = 0;
                atomicSub(&nact, 1);
            } else {
                if (W2 > W - W / 2) slack--;
                double s = r / (kf * E);
                const double h = 1.0 - 0.5 * s * (kd * (A / E));
                if (h >= 0.5 && h <= 2.0) s /= h;
                double xn = x - s;
                if (xn == x) xn = gl_unord(r < 0.0 ? gl_ord(x) + 1 : gl_ord(x) - 1);
                x = (slack > 0 && xn > lo && xn < hi) ? xn : gl_unord(gl_ord(lo) + W2 / 2);
                xs[t] = x;
            }
        }
        __syncthreads();
    }
    if (t < nl) {
        const bool up = !isnan(Fhi) && (isnan(Flo) || Fhi - q <= q - Flo);
        out[(size_t)t * P] = up ? hi : lo;
    }
}

// the blocks of one batch of bb targets, each with one byte count that the allocation and abc_glm_need share
struct GlBytes {
    size_t Z, wv, part1, part2, rec, tpk, row, seg, pf, pg, qs;
    size_t per_target() const { return Z + wv + part1 + part2 + rec + tpk + 3 * row + seg + pf + pg + qs; }
};
// sum: the call computes a summary (the four older entries: never, and their bytes are what they were)
GlBytes gl_bytes(size_t K, size_t n, size_t P, size_t G, bool sum) {
    const GlPlan pl = gl_plan(K);
    const size_t D = n + P, nchunk = (G + GL_GC - 1) / GL_GC;
    GlBytes y;
    y.Z = K * D * 8;
    y.wv = K * 8;
    y.part1 = pl.nch * (D + 3) * 8;
    y.part2 = pl.nch * D * D * 8;
    y.rec = GR_LEN * 8;
    y.tpk = K * P * 8;
    y.row = K * 8;
    y.seg = P * sizeof(GlSeg);
    y.pf = P * nchunk * 8;
    y.pg = P * nchunk * 4;
    y.qs = sum ? P * sizeof(GlQs) : 0;
    return y;
}
// targets per batch, from the bound nA of n so that the arena bound does not depend on the fit
size_t gl_batch(size_t K, size_t nA, size_t P, size_t G, size_t B, bool sum) {
    size_t bb = GL_BATCH_BYTES / gl_bytes(K, nA, P, G, sum).per_target();
    if (bb < 1) bb = 1;
    if (bb > GL_MAX_GRID_Y) bb = GL_MAX_GRID_Y;
    return bb < B ? bb : B;
}

GlOut gl_out(const abc_glm* m) {
    GlOut o;
    o.G = (int)m->G;
    o.cut = m->cut;
    o.dens = m->dens; o.lo_x = m->lo_x; o.step = m->step; o.mode = m->mode; o.mode_dens = m->mode_dens;
    o.mean = m->mean; o.var = m->var; o.ess = m->ess; o.log_md = m->log_md;
    o.C = m->C; o.c0 = m->c0; o.sigma_s = m->sigma_s; o.T = m->T; o.peaks = m->peaks; o.c = m->c;
    o.status = m->status;
    return o;
}

// Phi^-1(p), 0 < p < 1: Acklam's rational approximation (relative error 1.2e-9) and two of Halley's steps on erfc, in the lower half
// (p > 1/2: -Phi^-1(1 - p), whose argument is exact)
double gl_norm_inv(double p) {
    if (p > 0.5) return -gl_norm_inv(1.0 - p);
    static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                                1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                                6.680131188771972e+01, -1.328068155288572e+01};
    static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                                -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
    static const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
    double x;
    if (p < 0.02425) {
        const double q = sqrt(-2.0 * log(p));
        x = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
    } else {
        const double q = p - 0.5, r = q * q;
        x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
            (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
    }
    for (int i = 0; i < 2; i++) {
        const double e = 0.5 * erfc(-x * 0.7071067811865476) - p, u = e * 2.5066282746310002 * exp(0.5 * x * x);
        x -= u / (1.0 + 0.5 * x * u);
    }
    return x;
}

}  // namespace

size_t abc_glm_need(size_t B, size_t K, size_t P, size_t nA, size_t G, bool sum) {
    if (nA > GL_MAX) nA = GL_MAX;
    const size_t bb = gl_batch(K, nA, P, G, B, sum);
    return abc_density_segs_need(B, K, P) + bb * gl_bytes(K, nA, P, G, sum).per_target() + 16 * 256 + (sum ? 256 : 0);
}

// sv: the parameters' values and weights as the marginal density reads them (the bandwidths' rule); S, sld, Y, ldy, idx, om, w, O, KCO:
// as GlSrc; n <= 32 components, P <= 32; nA: the bound of n that abc_glm_need was asked with; sum: NULL, or the summary of a
// *_summary entry (checked by the caller: probs in host memory, every level strictly inside (0, 1))
int launch_glm(abc_ctx* ctx, const SmValues& sv, const double* S, size_t sld, const double* Y, size_t ldy, const uint64_t* idx,
               const double* om, const double* w, const double* O, int KCO, size_t B, size_t K, size_t P, size_t n, size_t nA,
               const abc_glm* glm, const abc_summary* sum, const char* fn) {
    if (nA > GL_MAX) nA = GL_MAX;
    const GlOut o = gl_out(glm);
    abc_density dn;
    memset(&dn, 0, sizeof(dn));
    dn.G = glm->G;
    dn.cut = glm->cut;
    dn.bw_scale = glm->bw_scale;
    dn.bw = glm->bw;
    const DnSeg* hseg = nullptr;
    ABC_TRY(launch_density_segs(ctx, sv, B, K, P, &dn, &hseg, fn));

    const size_t bb = gl_batch(K, nA, P, glm->G, B, sum != nullptr);
    const GlBytes y = gl_bytes(K, n, P, glm->G, sum != nullptr);
    const GlPlan pl = gl_plan(K);
    const int ni = (int)n, Pi = (int)P, D = ni + Pi, nchunk = (int)((glm->G + GL_GC - 1) / GL_GC);
    GlWs ws;
    ws.Z = (double*)abc_ws_alloc(ctx, bb * y.Z);
    ws.wv = (double*)abc_ws_alloc(ctx, bb * y.wv);
    ws.part1 = (double*)abc_ws_alloc(ctx, bb * y.part1);
    ws.part2 = (double*)abc_ws_alloc(ctx, bb * y.part2);
    ws.rec = (double*)abc_ws_alloc(ctx, bb * y.rec);
    ws.tpk = (double*)abc_ws_alloc(ctx, bb * y.tpk);
    ws.logc = (double*)abc_ws_alloc(ctx, bb * y.row);
    ws.logn = (double*)abc_ws_alloc(ctx, bb * y.row);
    ws.chat = (double*)abc_ws_alloc(ctx, bb * y.row);
    ws.seg = (GlSeg*)abc_ws_alloc(ctx, bb * y.seg);
    ws.pf = (double*)abc_ws_alloc(ctx, bb * y.pf);
    ws.pg = (int*)abc_ws_alloc(ctx, bb * y.pg);
    ws.qs = sum ? (GlQs*)abc_ws_alloc(ctx, bb * y.qs) : nullptr;
    if (sum && !ws.qs) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    GlSum sm = {nullptr, nullptr, nullptr};
    GlLev lv;
    memset(&lv, 0, sizeof(lv));
    if (sum) {
        sm.truth = sum->truth; sm.quant = sum->quant; sm.cdf = sum->cdf;
        if (sum->quant) {
            lv.nq = (int)sum->nq;
            for (int q = 0; q < lv.nq; q++) {
                lv.q[q] = sum->probs[q];
                lv.z[q] = gl_norm_inv(sum->probs[q]);
            }
        }
    }
    if (!ws.Z || !ws.wv || !ws.part1 || !ws.part2 || !ws.rec || !ws.tpk || !ws.logc || !ws.logn || !ws.chat || !ws.seg || !ws.pf || !ws.pg)
        ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    ABC_HIP(ctx, hipFuncSetAttribute((const void*)k_glm_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GL_SOLVE_LDS));
    GlSrc g;
    g.src = AjSrc{nullptr, n + P, S, sld, Y, ldy};
    g.idx = idx;
    g.om = om;
    g.w = w;
    g.O = O;
    g.KCO = KCO;
    const bool dens = o.dens || o.mode || o.mode_dens;
    for (size_t b0 = 0; b0 < B; b0 += bb) {
        const unsigned nb = (unsigned)((B - b0 < bb) ? B - b0 : bb);
        hipLaunchKernelGGL(k_glm_gather, dim3((unsigned)((K + 63) / 64), nb), dim3(256), 0, ctx->stream, g, K, ni, Pi, b0, ws);
        hipLaunchKernelGGL(k_glm_sums, dim3((unsigned)pl.nch, nb), dim3(256), 0, ctx->stream, K, D, pl.CH, ws);
        hipLaunchKernelGGL(k_glm_moments, dim3((unsigned)pl.nch, nb), dim3(256), 0, ctx->stream, K, D, pl.CH, ws);
        hipLaunchKernelGGL(k_glm_solve, dim3(nb), dim3(256), GL_SOLVE_LDS, ctx->stream, K, ni, Pi, pl.nch, b0, g, hseg, o, ws);
        ABC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_glm_peaks, dim3((unsigned)((K + GL_PB - 1) / GL_PB), nb), dim3(GL_PB), 0, ctx->stream, K, ni, Pi, b0, o, ws);
        hipLaunchKernelGGL(k_glm_evid, dim3((unsigned)((K + GL_EB - 1) / GL_EB), nb), dim3(GL_EB), 0, ctx->stream, K, ni, Pi, ws);
        hipLaunchKernelGGL(k_glm_weights, dim3(nb), dim3(256), 0, ctx->stream, K, ni, b0, o, ws);
        hipLaunchKernelGGL(k_glm_stats, dim3((unsigned)P, nb), dim3(256), 0, ctx->stream, K, Pi, b0, o, ws);
        ABC_HIP(ctx, hipGetLastError());
        if (sm.cdf) hipLaunchKernelGGL(k_glm_cdf, dim3((unsigned)P, nb), dim3(256), 0, ctx->stream, K, Pi, b0, sm, ws);
        if (sm.quant)
            hipLaunchKernelGGL(k_glm_quant, dim3((unsigned)(P * ((lv.nq + GL_QL - 1) / GL_QL)), nb), dim3(256), 0, ctx->stream, K, Pi, b0,
                               lv, sm, ws);
        if (sum) ABC_HIP(ctx, hipGetLastError());
        if (!dens) continue;
        hipLaunchKernelGGL(k_glm_dens, dim3((unsigned)(P * nchunk), nb), dim3(GL_BS), 0, ctx->stream, K, Pi, b0, nchunk, o, ws);
        if (nchunk > 1)
            hipLaunchKernelGGL(k_glm_mode, dim3((unsigned)((nb * P + 255) / 256)), dim3(256), 0, ctx->stream, (size_t)nb * P, b0 * P,
                               nchunk, o, ws);
        ABC_HIP(ctx, hipGetLastError());
    }
    return ABC_OK;
}

static_assert(GL_MAX == ABC_GLM_MAX, "limits of abc_glm_rank_targets_dev (api.hip checks them)");
