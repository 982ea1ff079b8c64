// Joint posterior of segments (abc_rank_targets_joint_dev, abc_weighted_joint_dev; the definition is in the header): the weighted
// means, covariances and correlations of a target's P parameters, and the two-dimensional Gaussian kernel density of chosen pairs
// of parameters on a G x G grid with its mode.  The values and weights of (target b, parameter j) are made by segment_dev.h, and
// the bandwidth, grid and kernel constants of every parameter by launch_density_segs (density.hip): the bits of the marginal
// densities.
//   k_jt_mean   one work-group per (b, j): W, S2 and sum w v.  Every thread adds its entries e = t, t + JT_BS, ... in ascending
//               order, then a fixed tree over the threads.  A bad parameter (NaN record) gets a NaN mean.
//   k_jt_cov    one work-group per (b, 16 x 16 tile of the upper triangle of tiles).  The deviations v - mean of the tile's 32
//               parameters are staged in LDS 64 entries at a time; thread (i, j) runs three fma chains over e ascending, for cov_ij
//               and for the two variances (the chain of cov_ii is the diagonal cell's own, so both see the same bits), and writes
//               cell (i, j) and its mirror.
//   k_jt_pair   the hot path, on the fp64 matrix pipe.  F = E_i diag(w) E_j', E_p[g, e] = exp(-((x_g - v_ep) / h_p)^2 / 2), is a
//               GEMM over the entries.  A wave owns a 64 x 64 block of the G x G output: sixteen v_mfma_f64_16x16x4_f64
//               accumulators (4 x 4 blocks of 16 x 16), of which only those with a row and a column below G are computed.  The
//               pair's (v_i, v_j, w) are staged in LDS in tiles of JT_TILE entries, padded with zero weights to a multiple of 4.
//               A step takes 4 entries: lane l reads entry e0 + (l >> 4) (four addresses per wave, broadcast) and forms, for
//               each of its four row blocks, the A element w_e E_i[16 rb + (l & 15), e] and, for each column block, the B element
//               E_j[16 cb + (l & 15), e] with dn_kern: 8 exponentials per 16 MFMAs.  Operand layout as gram.hip: A[row = l & 15]
//               [k = l >> 4], B[k = l >> 4][col = l & 15], C/D row = (l >> 4) + 4 r, col = l & 15.  Rows and columns at or past
//               G and entries past K are zero operands.  An accumulator chained through the MFMAs is the fma chain over e
//               ascending (project.hip), so a cell's sum depends on K only.  With G <= 64 a work-group is one wave; above, four
//               waves take four blocks of the pair and share the staging.  Every wave leaves its largest f (smallest flat index
//               g G + g' on ties, a fixed tree over the lanes) as a candidate; dens is written only when asked for and the mode
//               never reads it back.  Held to two waves per SIMD (203 registers): DESIGN.md 7e has the timings of both.
//   k_jt_mode   one thread per (b, pair): the candidates in block order, ties to the smaller flat index.
// No floating-point atomics; a target's outputs do not depend on the batch, nor a pair's on the other pairs.
#include <math.h>

#include "abc_internal.h"
#include "density_dev.h"
#include "segment_dev.h"

namespace {

constexpr int JT_BS = 256;                                  // threads of the moment kernels' work-groups
constexpr int JT_CT = 16;                                   // parameters per side of a covariance tile
constexpr int JT_CE = 64;                                   // entries of a covariance tile staged at a time
constexpr int JT_TILE = 1024;                               // entries of a pair staged in LDS at a time (a multiple of 4)
constexpr int JT_MIX = 7;                                   // vector instructions scheduled after each MFMA of a full block
constexpr unsigned JT_MAX_GRID_Y = 65535;
typedef double jd4 __attribute__((ext_vector_type(4)));

struct JtArgs {
    int G, npairs;
    double *mean, *cov, *corr, *dens, *mode, *mode_dens;
};

// grid (P, targets b0 + blockIdx.y); mu: B x P means, ws: B x 2 = W, S2.  HC (here, in k_jt_cov and in k_jt_pair): the values under
// the variance correction, an instance the launcher takes only when a.hcoef is set
template <bool HC>
__global__ __launch_bounds__(JT_BS) void k_jt_mean(SmArgs a, JtArgs d, size_t b0, const DnSeg* __restrict__ sp, double* __restrict__ mu,
                                                   double* __restrict__ ws) {
    __shared__ double r0[JT_BS], r1[JT_BS], r2[JT_BS];
    const int t = threadIdx.x, j = (int)blockIdx.x;
    const size_t b = b0 + blockIdx.y, sg = b * a.P + j, K = a.K;
    const SmSeg s = sm_seg<HC>(a, b, j);
    const bool bad = isnan(sp[sg].h);
    double W = 0.0, S2 = 0.0, A1 = 0.0;
    for (size_t e = t; e < K; e += JT_BS) {
        const double w = sm_weight(a, s, e);
        if (w > 0.0) {
            W += w;
            S2 = fma(w, w, S2);
            if (!bad) A1 = fma(w, sm_value<true, HC>(a, s, e), A1);
        }
    }
    r0[t] = W; r1[t] = S2; r2[t] = A1;
    __syncthreads();
    for (int st = JT_BS / 2; st > 0; st >>= 1) {
        if (t < st) {
            r0[t] += r0[t + st];
            r1[t] += r1[t + st];
            r2[t] += r2[t + st];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double m = bad ? dn_nan() : r2[0] / r0[0];
    mu[sg] = m;
    if (d.mean) d.mean[sg] = m;
    if (j == 0) {
        ws[2 * b] = r0[0];
        ws[2 * b + 1] = r1[0];
    }
}

// grid (tiles ti <= tj of 16 parameters, targets b0 + blockIdx.y); thread (il, jl) = (t >> 4, t & 15)
template <bool TF, bool HC>
__global__ __launch_bounds__(JT_BS) void k_jt_cov(SmArgs a, JtArgs d, size_t b0, const double* __restrict__ mu,
                                                  const double* __restrict__ ws) {
    __shared__ double dv[2 * JT_CT][JT_CE + 1];
    __shared__ double wt[JT_CE];
    const int t = threadIdx.x, P = a.P, nt = (P + JT_CT - 1) / JT_CT;
    int ti = 0, rest = (int)blockIdx.x;
    while (rest >= nt - ti) { rest -= nt - ti; ti++; }
    const int tj = ti + rest;
    const size_t b = b0 + blockIdx.y, K = a.K;
    const int il = t >> 4, jl = t & 15, i = JT_CT * ti + il, j = JT_CT * tj + jl;
    double cij = 0.0, cii = 0.0, cjj = 0.0;
    for (size_t base = 0; base < K; base += JT_CE) {
        const int len = (K - base < (size_t)JT_CE) ? (int)(K - base) : JT_CE;
        const int el = t & (JT_CE - 1);
        if (t < JT_CE) {
            double w = 0.0;
            if (el < len) {
                w = sm_weight(a, sm_seg(a, b, 0), base + (size_t)el);
                w = w > 0.0 ? w : 0.0;
            }
            wt[el] = w;
        }
        for (int c = t / JT_CE; c < 2 * JT_CT; c += JT_BS / JT_CE) {
            const int p = (c < JT_CT) ? JT_CT * ti + c : JT_CT * tj + (c - JT_CT);
            double v = 0.0;
            if (p < P && el < len) {
                const double m = mu[b * P + p];
                const SmSeg s = sm_seg<HC>(a, b, p);
                if (!isnan(m) && sm_weight(a, s, base + (size_t)el) > 0.0) v = sm_value<TF, HC>(a, s, base + (size_t)el) - m;
            }
            dv[c][el] = v;
        }
        __syncthreads();
        for (int e = 0; e < len; e++) {
            const double di = dv[il][e], dj = dv[JT_CT + jl][e], w = wt[e];
            const double wi = w * di;
            cij = fma(wi, dj, cij);
            cii = fma(wi, di, cii);
            cjj = fma(w * dj, dj, cjj);
        }
        __syncthreads();
    }
    if (i >= P || j >= P || i > j) return;
    const double W = ws[2 * b], S2 = ws[2 * b + 1], dn = W - S2 / W;
    const bool bad = isnan(mu[b * P + i]) || isnan(mu[b * P + j]);
    double cov = 0.0, vi = 0.0, vj = 0.0;
    if (dn > 0.0) {
        cov = cij / dn;
        vi = cii / dn;
        vj = cjj / dn;
    }
    double corr = dn_nan();
    if (vi > 0.0 && vj > 0.0) corr = (i == j) ? 1.0 : fmin(fmax(cov / (sqrt(vi) * sqrt(vj)), -1.0), 1.0);
    if (bad) cov = corr = dn_nan();
    const size_t o = b * (size_t)P * P, ij = o + (size_t)i * P + j, ji = o + (size_t)j * P + i;
    if (d.cov) { d.cov[ij] = cov; d.cov[ji] = cov; }
    if (d.corr) { d.corr[ij] = corr; d.corr[ji] = corr; }
}

// all pairs i < j in the order (0,1), (0,2), ...: one thread per i
__global__ __launch_bounds__(256) void k_jt_allpairs(int P, int* __restrict__ pairs) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= P - 1) return;
    size_t o = (size_t)i * (size_t)(2 * P - i - 1) / 2;        // pairs whose first index is below i
    for (int j = i + 1; j < P; j++, o++) {
        pairs[2 * o] = i;
        pairs[2 * o + 1] = j;
    }
}

// the operands of one step of 4 entries for a wave's block: lane l holds entry (l >> 4) of the step, row / column (l & 15) of each
// 16 x 16 block; FULL: all 16 blocks lie below G
template <bool FULL>
__device__ __forceinline__ void jt_ops(double (&av)[4], double (&bv)[4], const double (&x)[4], const double (&y)[4], double vi, double vj,
                                       double w, double ci, double cj, const bool (&rok)[4], const bool (&cok)[4]) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        av[r] = (FULL || rok[r]) ? w * dn_kern((x[r] - vi) * ci) : 0.0;
        bv[r] = (FULL || cok[r]) ? dn_kern((y[r] - vj) * cj) : 0.0;
    }
}

template <bool FULL>
__device__ __forceinline__ void jt_mma(jd4 (&acc)[4][4], const double (&av)[4], const double (&bv)[4], int nrb, int ncb) {
#pragma unroll
    for (int rb = 0; rb < 4; rb++)
#pragma unroll
        for (int cb = 0; cb < 4; cb++)
            if (FULL || (rb < nrb && cb < ncb))
                acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rb], bv[cb], acc[rb][cb], 0, 0, 0);
}

// grid (npairs x nchunk, targets b0 + blockIdx.y), NW waves; wave wv takes block chunk NW + wv of the nbx x nbx blocks of 64 x 64;
// pf / pg: the candidates [b][pair][block]
template <int NW, bool HC>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_jt_pair(SmArgs a, JtArgs d, size_t b0, const DnSeg* __restrict__ sp,
                                                     const double* __restrict__ ws, const int* __restrict__ pairs, int nbx, int nchunk,
                                                     double* __restrict__ pf, int* __restrict__ pg) {
    __shared__ double tvi[JT_TILE], tvj[JT_TILE], tw[JT_TILE];
    __shared__ double rf[64 * NW];
    __shared__ int rg[64 * NW];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, G = d.G, nblk = nbx * nbx;
    const int pr = (int)(blockIdx.x / (unsigned)nchunk), ch = (int)(blockIdx.x % (unsigned)nchunk);
    const int blk = ch * NW + wv;
    const bool live = blk < nblk;                              // (wave-uniform)
    const int bi = live ? blk / nbx : 0, bj = live ? blk % nbx : 0;
    const size_t b = b0 + blockIdx.y, K = a.K;
    const int pi = pairs[2 * pr], pj = pairs[2 * pr + 1];
    const SmSeg si = sm_seg<HC>(a, b, pi), sj = sm_seg<HC>(a, b, pj);
    const DnSeg qi = sp[b * a.P + pi], qj = sp[b * a.P + pj];
    const bool bad = isnan(qi.h) || isnan(qj.h);
    const int nrb = (G - 64 * bi + 15) / 16 < 4 ? (G - 64 * bi + 15) / 16 : 4;
    const int ncb = (G - 64 * bj + 15) / 16 < 4 ? (G - 64 * bj + 15) / 16 : 4;
    const bool full = 64 * bi + 64 <= G && 64 * bj + 64 <= G;
    double x[4], y[4];
    bool rok[4], cok[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int g = 64 * bi + 16 * r + (lane & 15), g2 = 64 * bj + 16 * r + (lane & 15);
        rok[r] = g < G;
        cok[r] = g2 < G;
        x[r] = fma((double)g, qi.step, qi.lo_x);
        y[r] = fma((double)g2, qj.step, qj.lo_x);
    }
    jd4 acc[4][4];
#pragma unroll
    for (int rb = 0; rb < 4; rb++)
#pragma unroll
        for (int cb = 0; cb < 4; cb++) acc[rb][cb] = (jd4){0.0, 0.0, 0.0, 0.0};
    if (!bad)
        for (size_t base = 0; base < K; base += JT_TILE) {
            const int len = (K - base < (size_t)JT_TILE) ? (int)(K - base) : JT_TILE;
            const int len4 = (len + 3) & ~3;
            for (int i = t; i < len4; i += 64 * NW) {
                double w = 0.0, vi = 0.0, vj = 0.0;
                if (i < len) {
                    const size_t e = base + (size_t)i;
                    w = sm_weight(a, si, e);
                    w = w > 0.0 ? w : 0.0;
                    vi = sm_value<true, HC>(a, si, e);
                    vj = sm_value<true, HC>(a, sj, e);
                }
                tvi[i] = vi; tvj[i] = vj; tw[i] = w;
            }
            __syncthreads();
            if (live) {
                double av[4], bv[4];
                if (full) {
                    // the operands of step s + 1 are formed between the MFMAs of step s (JT_MIX vector instructions after each),
                    // so that the exponentials run while the matrix pipe works; the last step forms its own once more, unused
                    // (the entry of step s + 2 is read from LDS a step earlier still)
                    const int i0 = lane >> 4, last = len4 - 4 + i0;
                    jt_ops<true>(av, bv, x, y, tvi[i0], tvj[i0], tw[i0], qi.c, qj.c, rok, cok);
                    int nx = i0 + 4 < last ? i0 + 4 : last;
                    double nvi = tvi[nx], nvj = tvj[nx], nw = tw[nx];
                    for (int i = i0; i < len4; i += 4) {
                        double an[4], bn[4];
                        jt_ops<true>(an, bn, x, y, nvi, nvj, nw, qi.c, qj.c, rok, cok);
                        nx = nx + 4 < last ? nx + 4 : last;
                        nvi = tvi[nx]; nvj = tvj[nx]; nw = tw[nx];
                        jt_mma<true>(acc, av, bv, 4, 4);
#pragma unroll
                        for (int k = 0; k < 16; k++) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);        // one MFMA
                            __builtin_amdgcn_sched_group_barrier(0x002, JT_MIX, 0);   // JT_MIX VALU
                        }
#pragma unroll
                        for (int r = 0; r < 4; r++) { av[r] = an[r]; bv[r] = bn[r]; }
                    }
                } else {
                    for (int i = lane >> 4; i < len4; i += 4) {
                        jt_ops<false>(av, bv, x, y, tvi[i], tvj[i], tw[i], qi.c, qj.c, rok, cok);
                        jt_mma<false>(acc, av, bv, nrb, ncb);
                    }
                }
            }
            __syncthreads();
        }
    // W 2 pi h_i h_j
    const double den = ws[2 * b] * 6.283185307179586 * qi.h * qj.h;
    const size_t o = (b * (size_t)d.npairs + pr) * (size_t)G * G;
    double bf = -1.0;
    int bg = 0x7fffffff;
    if (live) {
#pragma unroll
        for (int rb = 0; rb < 4; rb++)
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    const int g = 64 * bi + 16 * rb + (lane >> 4) + 4 * r, g2 = 64 * bj + 16 * cb + (lane & 15);
                    if (g < G && g2 < G) {
                        const double f = bad ? dn_nan() : acc[rb][cb][r] / den;
                        const int flat = g * G + g2;
                        if (d.dens) d.dens[o + flat] = f;
                        if (f > bf || (f == bf && flat < bg)) { bf = f; bg = flat; }
                    }
                }
    }
    if (!d.mode && !d.mode_dens) return;
    rf[t] = bf;
    rg[t] = bg;
    __syncthreads();
    for (int st = 32; st > 0; st >>= 1) {                      // (within the wave: lanes lane + st of the same wave)
        if (lane < st) {
            const double f2 = rf[t + st];
            const int g2 = rg[t + st];
            if (f2 > rf[t] || (f2 == rf[t] && g2 < rg[t])) { rf[t] = f2; rg[t] = g2; }
        }
        __syncthreads();
    }
    if (lane != 0 || !live) return;
    const size_t c = (b * (size_t)d.npairs + pr) * nblk + blk;
    pf[c] = rf[t];
    pg[c] = rg[t];
}

// the blocks' candidates of a (target, pair); one thread each
__global__ __launch_bounds__(256) void k_jt_mode(JtArgs d, int P, size_t n, const DnSeg* __restrict__ sp, const int* __restrict__ pairs,
                                                 int nblk, const double* __restrict__ pf, const int* __restrict__ pg) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const size_t b = c / (size_t)d.npairs;
    const int pr = (int)(c % (size_t)d.npairs);
    double bf = -1.0;
    int bg = 0x7fffffff;
    for (int k = 0; k < nblk; k++) {
        const double f = pf[c * nblk + k];
        const int g = pg[c * nblk + k];
        if (f > bf || (f == bf && g < bg)) { bf = f; bg = g; }
    }
    const DnSeg qi = sp[b * P + pairs[2 * pr]], qj = sp[b * P + pairs[2 * pr + 1]];
    const bool none = isnan(qi.h) || isnan(qj.h) || bg >= d.G * d.G;
    if (d.mode) {
        d.mode[2 * c] = none ? dn_nan() : fma((double)(bg / d.G), qi.step, qi.lo_x);
        d.mode[2 * c + 1] = none ? dn_nan() : fma((double)(bg % d.G), qj.step, qj.lo_x);
    }
    if (d.mode_dens) d.mode_dens[c] = none ? dn_nan() : bf;
}

}  // namespace

size_t abc_joint_pairs(const abc_joint* jt, size_t P) { return jt->pairs ? jt->npairs : P * (P - 1) / 2; }

size_t abc_joint_need(size_t B, size_t K, size_t P, size_t G, size_t npairs) {
    const size_t nbx = (G + 63) / 64;
    return abc_density_segs_need(B, K, P) + B * P * 8 + B * 16 + npairs * 8 + B * npairs * nbx * nbx * 12 + 8 * 256;
}

int launch_joint(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const abc_joint* jt, const char* fn) {
    if (B == 0 || K == 0 || P == 0) return ABC_OK;
    const size_t np = abc_joint_pairs(jt, P);
    const int G = (int)jt->G, nbx = (G + 63) / 64, nblk = nbx * nbx;
    abc_density dn;
    memset(&dn, 0, sizeof(dn));
    dn.G = jt->G;
    dn.cut = jt->cut;
    dn.bw_scale = jt->bw_scale;
    dn.bw = jt->bw;
    dn.grid = jt->grid;
    dn.bw_out = jt->bw_out;
    const DnSeg* sp = nullptr;
    ABC_TRY(launch_density_segs(ctx, sv, B, K, P, &dn, &sp, fn));
    JtArgs d;
    d.G = G;
    d.npairs = (int)np;
    d.mean = jt->mean;
    d.cov = jt->cov;
    d.corr = jt->corr;
    d.dens = jt->dens;
    d.mode = jt->mode;
    d.mode_dens = jt->mode_dens;
    const bool mode = d.mode || d.mode_dens, pair = np > 0 && (d.dens || mode), mom = d.mean || d.cov || d.corr;
    if (!pair && !mom) return ABC_OK;
    double* mu = (double*)abc_ws_alloc(ctx, B * P * 8);
    double* ws = (double*)abc_ws_alloc(ctx, B * 16);
    int* pairs = pair ? (int*)abc_ws_alloc(ctx, np * 8) : nullptr;
    double* pf = (pair && mode) ? (double*)abc_ws_alloc(ctx, B * np * nblk * 8) : nullptr;
    int* pg = (pair && mode) ? (int*)abc_ws_alloc(ctx, B * np * nblk * 4) : nullptr;
    if (!mu || !ws || (pair && !pairs) || (pair && mode && (!pf || !pg))) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    if (pair) {
        if (jt->pairs) {
            ABC_HIP(ctx, hipMemcpyAsync(pairs, jt->pairs, np * 8, hipMemcpyHostToDevice, ctx->stream));
        } else {
            hipLaunchKernelGGL(k_jt_allpairs, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, (int)P, pairs);
            ABC_HIP(ctx, hipGetLastError());
        }
    }
    const SmArgs a = sm_args(sv, K, P);
    const size_t nt = (P + JT_CT - 1) / JT_CT;
    const int nchunk = G <= 64 ? 1 : (nblk + 3) / 4;
    for (size_t b0 = 0; b0 < B; b0 += JT_MAX_GRID_Y) {
        const size_t nb = (B - b0 < JT_MAX_GRID_Y) ? B - b0 : JT_MAX_GRID_Y;
        hipLaunchKernelGGL(a.hcoef ? k_jt_mean<true> : k_jt_mean<false>, dim3((unsigned)P, (unsigned)nb), dim3(JT_BS), 0, ctx->stream, a, d, b0, sp, mu, ws);
        ABC_HIP(ctx, hipGetLastError());
        if (d.cov || d.corr) {
            // (the back-transform costs k_jt_cov a wave per SIMD: calls without transforms keep the instance without it)
            // (the variance correction's exponential likewise: one instance with both, under that setting only)
            const auto cov = a.hcoef ? k_jt_cov<true, true> : a.tf.kind ? k_jt_cov<true, false> : k_jt_cov<false, false>;
            hipLaunchKernelGGL(cov, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)nb), dim3(JT_BS), 0, ctx->stream, a, d, b0,
                               (const double*)mu, (const double*)ws);
            ABC_HIP(ctx, hipGetLastError());
        }
        if (!pair) continue;
        const dim3 grid((unsigned)(np * nchunk), (unsigned)nb);
        const auto pair1 = a.hcoef ? k_jt_pair<1, true> : k_jt_pair<1, false>;
        const auto pair4 = a.hcoef ? k_jt_pair<4, true> : k_jt_pair<4, false>;
        if (G <= 64)
            hipLaunchKernelGGL(pair1, grid, dim3(64), 0, ctx->stream, a, d, b0, sp, (const double*)ws, (const int*)pairs, nbx, nchunk,
                               pf, pg);
        else
            hipLaunchKernelGGL(pair4, grid, dim3(256), 0, ctx->stream, a, d, b0, sp, (const double*)ws, (const int*)pairs, nbx, nchunk,
                               pf, pg);
        ABC_HIP(ctx, hipGetLastError());
    }
    if (pair && mode) {
        const size_t n = B * np;
        hipLaunchKernelGGL(k_jt_mode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d, (int)P, n, sp, (const int*)pairs,
                           nblk, (const double*)pf, (const int*)pg);
        ABC_HIP(ctx, hipGetLastError());
    }
    return ABC_OK;
}
