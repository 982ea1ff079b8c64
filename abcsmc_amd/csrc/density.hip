// Weighted posterior densities and modes of segments (abc_rank_targets_density_dev, abc_weighted_density_dev; the definition is in
// the header).  A segment is one (target b, parameter j); its K values and weights are made by segment_dev.h, the same bits the
// summaries sort.
//   quantiles   Q(0), Q(0.25), Q(0.75), Q(1) of every segment by launch_summary (summary.hip) into workspace: u_min, the IQR, u_max;
//               all four are NaN exactly when the segment holds a non-finite value
//   k_dn_moments  one work-group per segment: W, S2 and the sum of w (v - u_min) in one pass, the centred sum about the mean in a
//               second; every thread adds its entries e = t, t + DN_BS, ... in ascending order, then a fixed tree over the threads.
//               Thread 0 makes h (or takes the given one), lo_x, step and the kernel's constants (DnSeg, NaN for a bad segment).
//   k_dn_dens   the hot path.  Work-groups over (segment, chunk of DN_GC grid points); a thread holds DN_R grid points in registers
//               (g = chunk DN_GC + r DN_BS + t, so the stores coalesce).  The segment's (v_e, w_e) are staged in LDS in tiles of
//               DN_TILE entries; every lane reads the same entry (a broadcast, no bank conflicts) and one read feeds DN_R kernel
//               evaluations.  The sum of a grid point is one fma chain over e ascending, whatever the tile, so it depends on K only.
//               The work-group's largest f (smallest g on ties) is found by a fixed tree; with one chunk it is the mode, otherwise
//               k_dn_mode takes the chunks' candidates in chunk order.  dens is written only when asked for, and the mode never
//               reads it back.
// launch_density_segs is the first half (the bandwidth check, the quantiles, k_dn_moments) on its own: the pair densities of
// joint.hip start from the same records, and density_dev.h holds what the two files share on the device (DnSeg, dn_kern).
// Kernel evaluation (dn_kern, density_dev.h): the argument t = -((x - v) c)^2, c = sqrt(log2(e) / 2) / h, is formed in fp64; 2^t is split as
// 2^n 2^(t - n) with n = rint(t), and only the factor 2^(t - n), |t - n| <= 1/2, is taken in f32 (v_exp_f32), then scaled by
// v_ldexp_f64.  Relative error of a term about 1e-7 (the f32 exponential's rounding), inside the header's 1e-6 contract;
// -DDN_EXP_FP64 builds the plain fp64 exp2 instead (DESIGN.md has both timings).
// No floating-point atomics; a target's outputs do not depend on the batch.
#include <math.h>

#include "abc_internal.h"
#include "density_dev.h"
#include "segment_dev.h"

namespace {

constexpr int DN_BS = 256;                                  // threads of every density work-group
constexpr int DN_R = 2;                                     // grid points per thread
constexpr int DN_GC = DN_BS * DN_R;                         // grid points per work-group
constexpr int DN_TILE = 1024;                               // entries staged in LDS at a time
constexpr unsigned DN_MAX_GRID_Y = 65535;

struct DnArgs {
    int G;
    double cut, bw_scale;
    const double* bw;
    double *dens, *grid, *bw_out, *mode, *mode_dens;
};

// grid (P, targets b0 + blockIdx.y); q4: B x 4 x P quantiles at 0, 0.25, 0.75, 1.  HC: the values under the variance correction
// (taken by the launcher only when a.hcoef is set, here and in k_dn_dens)
template <bool HC>
__global__ __launch_bounds__(DN_BS) void k_dn_moments(SmArgs a, DnArgs d, size_t b0, const double* __restrict__ q4,
                                                      DnSeg* __restrict__ sp) {
    __shared__ double r0[DN_BS], r1[DN_BS], r2[DN_BS];
    __shared__ unsigned rf[DN_BS];
    const int t = threadIdx.x, j = (int)blockIdx.x;
    const size_t b = b0 + blockIdx.y, sg = b * a.P + j, K = a.K;
    const SmSeg s = sm_seg<HC>(a, b, j);
    const double* q = q4 + b * 4 * (size_t)a.P + j;
    const double umin = q[0], q25 = q[a.P], q75 = q[2 * (size_t)a.P], umax = q[3 * (size_t)a.P];
    const bool bad = isnan(umin);
    double W = 0.0, S2 = 0.0, A1 = 0.0;
    unsigned first = 0xFFFFFFFFu;
    if (!bad)
        for (size_t e = t; e < K; e += DN_BS) {
            const double w = sm_weight(a, s, e);
            if (w > 0.0) {
                const double v = sm_value<true, HC>(a, s, e);
                W += w;
                S2 = fma(w, w, S2);
                A1 = fma(w, v - umin, A1);
                if (first == 0xFFFFFFFFu) first = (unsigned)e;
            }
        }
    r0[t] = W; r1[t] = S2; r2[t] = A1; rf[t] = first;
    __syncthreads();
    for (int st = DN_BS / 2; st > 0; st >>= 1) {
        if (t < st) {
            r0[t] += r0[t + st];
            r1[t] += r1[t + st];
            r2[t] += r2[t + st];
            rf[t] = rf[t] < rf[t + st] ? rf[t] : rf[t + st];
        }
        __syncthreads();
    }
    W = r0[0]; S2 = r1[0];
    const double moff = r2[0] / W;                             // mean - umin
    first = rf[0];
    __syncthreads();
    double C2 = 0.0;
    if (!bad)
        for (size_t e = t; e < K; e += DN_BS) {
            const double w = sm_weight(a, s, e);
            if (w > 0.0) {
                const double dv = (sm_value<true, HC>(a, s, e) - umin) - moff;
                C2 = fma(w, dv * dv, C2);
            }
        }
    r0[t] = C2;
    __syncthreads();
    for (int st = DN_BS / 2; st > 0; st >>= 1) {
        if (t < st) r0[t] += r0[t + st];
        __syncthreads();
    }
    if (t != 0) return;
    DnSeg p;
    p.h = p.lo_x = p.step = p.den = p.c = dn_nan();
    if (!bad) {
        double h;
        if (d.bw) {
            h = d.bw[sg];
        } else {
            const double dn = W - S2 / W;
            const double sd = dn > 0.0 ? sqrt(r0[0] / dn) : 0.0;
            const double neff = W * W / S2;
            double lo = fmin(sd, (q75 - q25) / 1.34);
            if (lo == 0.0) lo = sd;
            if (lo == 0.0) lo = fabs(sm_value<true, HC>(a, s, (size_t)first));
            if (lo == 0.0) lo = 1.0;
            h = d.bw_scale * 0.9 * lo * pow(neff, -0.2);
        }
        p.h = h;
        p.lo_x = umin - d.cut * h;
        p.step = ((umax + d.cut * h) - p.lo_x) / (double)(d.G - 1);
        p.den = W * h * 2.5066282746310002;                    // sqrt(2 pi)
        p.c = 0.8493218002880191 / h;                          // sqrt(log2(e) / 2)
    }
    sp[sg] = p;
    if (d.bw_out) d.bw_out[sg] = p.h;
    if (d.grid) {
        d.grid[2 * sg] = p.lo_x;
        d.grid[2 * sg + 1] = p.step;
    }
}

// grid (P x nchunk, targets b0 + blockIdx.y); pf / pg: the chunks' candidates [segment][chunk] (nchunk > 1)
template <bool TF, bool HC>
__global__ __launch_bounds__(DN_BS) void k_dn_dens(SmArgs a, DnArgs d, size_t b0, const DnSeg* __restrict__ sp, int nchunk,
                                                   double* __restrict__ pf, int* __restrict__ pg) {
    __shared__ __attribute__((aligned(16))) double2 tile[DN_TILE];
    __shared__ double rf[DN_BS];
    __shared__ int rg[DN_BS];
    const int t = threadIdx.x, j = (int)(blockIdx.x % (unsigned)a.P), c = (int)(blockIdx.x / (unsigned)a.P), G = d.G;
    const size_t b = b0 + blockIdx.y, sg = b * a.P + j, K = a.K;
    const SmSeg s = sm_seg<HC>(a, b, j);
    const DnSeg p = sp[sg];
    const bool bad = isnan(p.h);
    double x[DN_R], acc[DN_R];
#pragma unroll
    for (int r = 0; r < DN_R; r++) {
        x[r] = fma((double)(c * DN_GC + r * DN_BS + t), p.step, p.lo_x);
        acc[r] = 0.0;
    }
    if (!bad)
        for (size_t base = 0; base < K; base += DN_TILE) {
            const int len = (K - base < (size_t)DN_TILE) ? (int)(K - base) : DN_TILE;
            for (int i = t; i < len; i += DN_BS) {
                const size_t e = base + (size_t)i;
                const double w = sm_weight(a, s, e);
                tile[i] = make_double2(sm_value<TF, HC>(a, s, e), w > 0.0 ? w : 0.0);
            }
            __syncthreads();
#pragma unroll 4
            for (int i = 0; i < len; i++) {
                const double2 vw = tile[i];
#pragma unroll
                for (int r = 0; r < DN_R; r++) acc[r] = fma(vw.y, dn_kern((x[r] - vw.x) * p.c), acc[r]);
            }
            __syncthreads();
        }
    double bf = -1.0;
    int bg = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < DN_R; r++) {                           // g ascending in r: a tie keeps the smaller g
        const int g = c * DN_GC + r * DN_BS + t;
        const double f = bad ? dn_nan() : acc[r] / p.den;
        if (g < G) {
            if (d.dens) d.dens[sg * (size_t)G + g] = f;
            if (f > bf) { bf = f; bg = g; }
        }
    }
    if (!d.mode && !d.mode_dens) return;
    rf[t] = bf;
    rg[t] = bg;
    __syncthreads();
    for (int st = DN_BS / 2; st > 0; st >>= 1) {
        if (t < st) {
            const double f2 = rf[t + st];
            const int g2 = rg[t + st];
            if (f2 > rf[t] || (f2 == rf[t] && g2 < rg[t])) { rf[t] = f2; rg[t] = g2; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    if (nchunk > 1) {
        pf[sg * nchunk + c] = rf[0];
        pg[sg * nchunk + c] = rg[0];
        return;
    }
    const bool none = bad || rg[0] >= G;
    if (d.mode) d.mode[sg] = none ? dn_nan() : fma((double)rg[0], p.step, p.lo_x);
    if (d.mode_dens) d.mode_dens[sg] = none ? dn_nan() : rf[0];
}

// the chunks' candidates in chunk order (g ascending: a tie keeps the earlier chunk); one thread per segment
__global__ __launch_bounds__(256) void k_dn_mode(DnArgs d, size_t nseg, const DnSeg* __restrict__ sp, int nchunk,
                                                 const double* __restrict__ pf, const int* __restrict__ pg) {
    const size_t sg = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (sg >= nseg) return;
    double bf = -1.0;
    int bg = 0x7fffffff;
    for (int c = 0; c < nchunk; c++) {
        const double f = pf[sg * nchunk + c];
        if (f > bf) { bf = f; bg = pg[sg * nchunk + c]; }
    }
    const DnSeg p = sp[sg];
    const bool none = isnan(p.h) || bg >= d.G;
    if (d.mode) d.mode[sg] = none ? dn_nan() : fma((double)bg, p.step, p.lo_x);
    if (d.mode_dens) d.mode_dens[sg] = none ? dn_nan() : bf;
}

// given bandwidths: *flag |= 1 for one that is not finite and positive
__global__ __launch_bounds__(256) void k_dn_bwcheck(const double* __restrict__ bw, size_t n, int* __restrict__ flag) {
    int badv = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double v = bw[i];
        if (!(v > 0.0) || !isfinite(v)) badv = 1;
    }
    if (badv) atomicOr(flag, 1);
}

const double DN_PROBS[4] = {0.0, 0.25, 0.75, 1.0};

DnArgs dn_args(const abc_density* dn) {
    DnArgs d;
    d.G = (int)dn->G;
    d.cut = dn->cut;
    d.bw_scale = dn->bw_scale;
    d.bw = dn->bw;
    d.dens = dn->dens;
    d.grid = dn->grid;
    d.bw_out = dn->bw_out;
    d.mode = dn->mode;
    d.mode_dens = dn->mode_dens;
    return d;
}

}  // namespace

size_t abc_density_segs_need(size_t B, size_t K, size_t P) {
    const size_t ns = B * P;
    return abc_summary_need(B, K, P) + ns * 4 * 8 + ns * sizeof(DnSeg) + 8 * 256;
}

size_t abc_density_need(size_t B, size_t K, size_t P, size_t G) {
    const size_t ns = B * P, nchunk = (G + DN_GC - 1) / DN_GC;
    return abc_density_segs_need(B, K, P) + ns * nchunk * 12 + 8 * 256;
}

int launch_density_segs(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const abc_density* dn, const DnSeg** segs,
                        const char* fn) {
    const size_t ns = B * P;
    if (dn->bw) {     // (synchronises, as the generic weights' check)
        int* flag = (int*)abc_ws_alloc(ctx, sizeof(int));
        if (!flag) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        ABC_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
        size_t blocks = (ns + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(k_dn_bwcheck, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, dn->bw, ns, flag);
        ABC_HIP(ctx, hipGetLastError());
        int h = 0;
        ABC_HIP(ctx, hipMemcpyAsync(&h, flag, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (h) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: a given bandwidth is not finite and positive", fn);
    }
    double* q4 = (double*)abc_ws_alloc(ctx, ns * 4 * 8);
    DnSeg* sp = (DnSeg*)abc_ws_alloc(ctx, ns * sizeof(DnSeg));
    if (!q4 || !sp) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    abc_summary s4;
    memset(&s4, 0, sizeof(s4));
    s4.probs = DN_PROBS;
    s4.nq = 4;
    s4.quant = q4;
    ABC_TRY(launch_summary(ctx, sv, B, K, P, &s4));
    const SmArgs a = sm_args(sv, K, P);
    const DnArgs d = dn_args(dn);
    for (size_t b0 = 0; b0 < B; b0 += DN_MAX_GRID_Y) {
        const size_t nb = (B - b0 < DN_MAX_GRID_Y) ? B - b0 : DN_MAX_GRID_Y;
        hipLaunchKernelGGL(a.hcoef ? k_dn_moments<true> : k_dn_moments<false>, dim3((unsigned)P, (unsigned)nb), dim3(DN_BS), 0,
                           ctx->stream, a, d, b0, (const double*)q4, sp);
        ABC_HIP(ctx, hipGetLastError());
    }
    *segs = sp;
    return ABC_OK;
}

int launch_density(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const abc_density* dn, const char* fn) {
    if (B == 0 || K == 0 || P == 0) return ABC_OK;
    const size_t ns = B * P;
    const int G = (int)dn->G, nchunk = (G + DN_GC - 1) / DN_GC;
    const DnSeg* sp = nullptr;
    ABC_TRY(launch_density_segs(ctx, sv, B, K, P, dn, &sp, fn));
    const SmArgs a = sm_args(sv, K, P);
    const DnArgs d = dn_args(dn);
    const bool mode = d.mode || d.mode_dens;
    if (!d.dens && !mode) return ABC_OK;
    double* pf = nullptr;
    int* pg = nullptr;
    if (nchunk > 1) {
        pf = (double*)abc_ws_alloc(ctx, ns * nchunk * 8);
        pg = (int*)abc_ws_alloc(ctx, ns * nchunk * 4);
        if (!pf || !pg) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    }
    for (size_t b0 = 0; b0 < B; b0 += DN_MAX_GRID_Y) {
        const size_t nb = (B - b0 < DN_MAX_GRID_Y) ? B - b0 : DN_MAX_GRID_Y;
        // (the back-transform costs k_dn_dens a wave per SIMD: calls without transforms keep the instance without it)
        // (so does the variance correction's exponential: one instance with both, taken only under that setting)
        const auto dens = a.hcoef ? k_dn_dens<true, true> : a.tf.kind ? k_dn_dens<true, false> : k_dn_dens<false, false>;
        hipLaunchKernelGGL(dens, dim3((unsigned)(P * nchunk), (unsigned)nb), dim3(DN_BS), 0, ctx->stream, a, d, b0, sp, nchunk, pf, pg);
        ABC_HIP(ctx, hipGetLastError());
    }
    if (mode && nchunk > 1) {
        hipLaunchKernelGGL(k_dn_mode, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, ctx->stream, d, ns, sp, nchunk,
                           (const double*)pf, (const int*)pg);
        ABC_HIP(ctx, hipGetLastError());
    }
    return ABC_OK;
}
