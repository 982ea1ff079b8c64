// Posterior draws of segments (abc_rank_targets_draws_dev, abc_weighted_draws_dev; the definition is in the header): S rows of a
// target's K entries resampled with the entries' weights (the weighted bootstrap) and, when smoothing, jittered by h_j z_j with the
// bandwidths of the marginal densities (the smoothed bootstrap: a sample of the estimate that density.hip draws).  The values and
// weights of (target b, parameter j) are made by segment_dev.h, the bandwidths by launch_density_segs (density.hip), the selection
// word and the deviates by philox_dev.h: the generator of the proposals, keyed by the descriptor's seed.
//   k_dr_cdf    one work-group per target: the inclusive prefix sums c_e of the weights, DR_CH entries at a time.  A chunk is a
//               fixed tree of serial sums: a thread adds its DR_R consecutive entries, one thread per group of DR_GT threads adds
//               the group's thread totals, thread 0 adds the DR_BS / DR_GT group totals, and c_e = carry + (group offset + (thread
//               offset + the thread's own prefix)); the carry is the chunk's last c.  Every level's offsets are the running sums
//               of the level below and a unit's total is its last prefix, so c_e >= c_{e-1} always and c_e == c_{e-1} exactly when
//               w_e == 0, whatever the rounding: the search below cannot stop at an entry of weight 0.  With equal weights every
//               sum is an integer and c_e = e + 1.  S2 is every thread's fma chain over its entries ascending, then a fixed tree
//               over the threads; ess = c_{K-1}^2 / S2.  The order depends on K only.  Segments with equal weights by
//               construction (method 0 without row importance weights, generic without w) are not scanned: ess = K.
//   k_dr_draw   the hot path.  A work-group takes DR_DB consecutive draws of a target.  First a thread per draw makes the
//               selection block, u and tau = u W, and finds src by binary search in the target's c (K doubles that every
//               work-group of the target reads: L2 hits after the first); floor(u K) for the unscanned segments.  src goes to LDS.
//               Then the threads run over (draw, group of four parameters): one Philox block gives the four deviates, the four
//               values are made by sm_value (method 1: the adjusted row in registers, as summary.hip and density.hip make it;
//               theta is not written) and go to an LDS tile laid out as draws is ([s][j]).  The tile holds DR_TILE doubles
//               (32 KiB: four work-groups per CU), that is DR_TILE / P draws at a time; it is then written out by consecutive
//               threads to consecutive addresses, 512 contiguous bytes per wave store, whatever P is.
// No floating-point atomics; a draw depends on (seed, stream id, s) and its target's segment only.
#include <math.h>

#include "abc_internal.h"
#include "density_dev.h"
#include "philox_dev.h"
#include "segment_dev.h"

namespace {

constexpr int DR_BS = 256;                                  // threads of both kernels' work-groups
constexpr int DR_R = 4;                                     // consecutive entries a thread sums in a chunk
constexpr int DR_CH = DR_BS * DR_R;                         // entries per chunk of the scan
constexpr int DR_GT = 16;                                   // threads per group of the scan's tree
constexpr int DR_NG = DR_BS / DR_GT;                        // groups
constexpr int DR_DB = 256;                                  // draws per work-group
constexpr int DR_TILE = 4096;                               // doubles of the output tile in LDS
constexpr unsigned DR_MAX_GRID_Y = 65535;
static_assert(DR_DB == DR_BS, "one thread per draw makes the selection");
static_assert(DR_TILE >= 1024, "the tile holds at least one draw of the largest P");

struct DrArgs {
    size_t S;
    uint32_t k0, k1;
    const uint64_t* stream;                                 // B stream ids (device) or NULL: b
    const double* c;                                        // B x K cumulative weights or NULL: equal weights
    double* draws;
    uint64_t* src;
    double* ess;
};

// grid (1, targets b0 + blockIdx.y); c: B x K or NULL (equal weights by construction: only ess is written)
__global__ __launch_bounds__(DR_BS) void k_dr_cdf(SmArgs a, size_t b0, double* __restrict__ c, double* __restrict__ ess) {
    __shared__ double tt[DR_BS], to[DR_BS], gt[DR_NG], go[DR_NG];
    __shared__ double carry_s;
    const int t = threadIdx.x;
    const size_t b = b0 + blockIdx.y, K = a.K;
    if (!c) {
        if (t == 0 && ess) ess[b] = (double)K;
        return;
    }
    const SmSeg s = sm_seg(a, b, 0);
    double* cb = c + b * K;
    double carry = 0.0, S2 = 0.0;
    for (size_t base = 0; base < K; base += DR_CH) {
        const size_t e0 = base + (size_t)t * DR_R;
        double l[DR_R], run = 0.0;
#pragma unroll
        for (int r = 0; r < DR_R; r++) {
            double w = 0.0;
            if (e0 + r < K) {
                w = sm_weight(a, s, e0 + r);
                w = w > 0.0 ? w : 0.0;
            }
            run += w;
            l[r] = run;
            S2 = fma(w, w, S2);
        }
        tt[t] = run;
        __syncthreads();
        if (t < DR_NG) {                                       // the thread offsets of group t and the group's total
            double o = 0.0;
            for (int k = 0; k < DR_GT; k++) {
                to[t * DR_GT + k] = o;
                o += tt[t * DR_GT + k];
            }
            gt[t] = o;
        }
        __syncthreads();
        if (t == 0) {                                          // the group offsets and the chunk's last c
            double o = 0.0;
            for (int g = 0; g < DR_NG; g++) {
                go[g] = o;
                o += gt[g];
            }
            carry_s = carry + o;
        }
        __syncthreads();
        const double off = go[t / DR_GT], mine = to[t];
#pragma unroll
        for (int r = 0; r < DR_R; r++)
            if (e0 + r < K) cb[e0 + r] = carry + (off + (mine + l[r]));
        carry = carry_s;
        __syncthreads();
    }
    if (!ess) return;
    tt[t] = S2;
    __syncthreads();
    for (int st = DR_BS / 2; st > 0; st >>= 1) {
        if (t < st) tt[t] += tt[t + st];
        __syncthreads();
    }
    if (t == 0) ess[b] = carry * carry / tt[0];
}

// grid (blocks of DR_DB draws, targets b0 + blockIdx.y); sp: the segments' records (SMOOTH)
// HC: the values under the variance correction (the launcher takes it only when a.hcoef is set)
template <bool SMOOTH, bool HC>
__global__ __launch_bounds__(DR_BS) void k_dr_draw(SmArgs a, DrArgs d, size_t b0, const DnSeg* __restrict__ sp) {
    __shared__ double tile[DR_TILE];
    __shared__ unsigned ssrc[DR_DB];
    const int t = threadIdx.x, P = a.P;
    const size_t b = b0 + blockIdx.y, K = a.K, S = d.S, s0 = (size_t)blockIdx.x * DR_DB;
    const int nd = (S - s0 < (size_t)DR_DB) ? (int)(S - s0) : DR_DB;
    const uint64_t id = d.stream ? d.stream[b] : (uint64_t)b;
    U4 ctr;
    ctr.x = (uint32_t)id;
    ctr.y = (uint32_t)(id >> 32);
    if (t < nd) {
        ctr.z = (uint32_t)(s0 + t);
        ctr.w = 0u;
        const U4 r = philox(ctr, d.k0, d.k1);
        const uint64_t m = ((uint64_t)r.x << 21) | (uint64_t)(r.y >> 11);
        const double u = (double)m * 1.1102230246251565e-16;  // 2^-53: exact, u in [0, 1)
        size_t e;
        if (d.c) {
            const double* __restrict__ cb = d.c + b * K;
            const double tau = u * cb[K - 1];
            size_t lo = 0, hi = K - 1;                         // c[hi] > tau: tau < W for every u < 1
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (cb[mid] > tau) hi = mid;
                else lo = mid + 1;
            }
            e = lo;
        } else {
            e = (size_t)(u * (double)K);
            if (e > K - 1) e = K - 1;
        }
        ssrc[t] = (unsigned)e;                                 // (K < 2^32 in every entry)
        if (d.src) d.src[b * S + s0 + t] = (uint64_t)e;
    }
    if (!d.draws) return;
    __syncthreads();
    const SmSeg seg0 = sm_seg(a, b, 0);
    const int nq = (P + 3) / 4, per = DR_TILE / P;             // draws per pass (P <= 1024: at least 4)
    double* __restrict__ out = d.draws + (b * S + s0) * (size_t)P;
    for (int p0 = 0; p0 < nd; p0 += per) {
        const int np = nd - p0 < per ? nd - p0 : per;
        for (int f = t; f < np * nq; f += DR_BS) {
            const int sl = f / nq, q = f - sl * nq;
            const size_t e = (size_t)ssrc[p0 + sl];
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            if (SMOOTH) {
                ctr.z = (uint32_t)(s0 + p0 + sl);
                ctr.w = 1u + (uint32_t)q;
                normal4(philox(ctr, d.k0, d.k1), z);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = 4 * q + k;
                if (j < P) {
                    SmSeg sj = seg0;                           // sm_seg(a, b, j): the members that depend on j
                    sj.j = j;
                    if (a.method == 1) sj.beta = seg0.beta + j;
                    if constexpr (HC) sm_seg_hc(a, sj);
                    double v = sm_value<true, HC>(a, sj, e);
                    if (SMOOTH) v = fma(sp[b * P + j].h, z[k], v);
                    tile[sl * P + j] = v;
                }
            }
        }
        __syncthreads();
        for (int i = t; i < np * P; i += DR_BS) out[(size_t)p0 * P + i] = tile[i];
        __syncthreads();
    }
}

// under row importance weights only: a target whose weights are all 0 (its last cumulative weight is not positive) has nothing to
// draw from: its draws become NaN, its src and ess 0.  Grid (blocks of 256 draws, targets b0 + blockIdx.y); the other targets are
// not touched.
__global__ __launch_bounds__(256) void k_dr_void(const double* __restrict__ c, size_t K, size_t S, int P, size_t b0,
                                                 double* __restrict__ draws, uint64_t* __restrict__ src, double* __restrict__ ess) {
    const size_t b = b0 + blockIdx.y;
    if (c[b * K + K - 1] > 0.0) return;                        // (uniform)
    const size_t s0 = (size_t)blockIdx.x * 256, s = s0 + threadIdx.x;
    if (ess && blockIdx.x == 0 && threadIdx.x == 0) ess[b] = 0.0;
    if (src && s < S) src[b * S + s] = 0;
    if (draws) {
        const size_t n = (S - s0 < 256 ? S - s0 : 256) * (size_t)P;
        for (size_t i = threadIdx.x; i < n; i += 256) draws[(b * S + s0) * (size_t)P + i] = dn_nan();
    }
}

__global__ __launch_bounds__(256) void k_dr_nan(double* __restrict__ x, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = dn_nan();
}

}  // namespace

size_t abc_draws_need(size_t B, size_t K, size_t P, int smooth) {
    return (smooth ? abc_density_segs_need(B, K, P) : 0) + B * K * 8 + B * 8 + 8 * 256;
}

int launch_draws(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const abc_draws* dr, const char* fn) {
    if (B == 0 || K == 0 || P == 0) return ABC_OK;
    const DnSeg* sp = nullptr;
    if (dr->smooth) {     // the bandwidths of the marginal densities (neither h nor bw_out depends on the grid)
        abc_density dn;
        memset(&dn, 0, sizeof(dn));
        dn.G = 2;
        dn.bw_scale = dr->bw_scale;
        dn.bw = dr->bw;
        dn.bw_out = dr->bw_out;
        ABC_TRY(launch_density_segs(ctx, sv, B, K, P, &dn, &sp, fn));
    } else if (dr->bw_out) {
        hipLaunchKernelGGL(k_dr_nan, dim3((unsigned)((B * P + 255) / 256)), dim3(256), 0, ctx->stream, dr->bw_out, B * P);
        ABC_HIP(ctx, hipGetLastError());
    }
    const bool weighted = sv.method == 1 || (sv.method == 2 && sv.w) || (sv.method == 0 && sv.om);   // (om: row importance weights)
    const bool select = dr->draws || dr->src;
    if (!select && !dr->ess) return ABC_OK;
    double* c = weighted ? (double*)abc_ws_alloc(ctx, B * K * 8) : nullptr;
    uint64_t* stream = (dr->stream && select) ? (uint64_t*)abc_ws_alloc(ctx, B * 8) : nullptr;
    if ((weighted && !c) || (dr->stream && select && !stream)) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    if (stream) ABC_HIP(ctx, hipMemcpyAsync(stream, dr->stream, B * 8, hipMemcpyHostToDevice, ctx->stream));
    const SmArgs a = sm_args(sv, K, P);
    DrArgs d;
    d.S = dr->S;
    d.k0 = (uint32_t)dr->seed;
    d.k1 = (uint32_t)(dr->seed >> 32);
    d.stream = stream;
    d.c = c;
    d.draws = dr->draws;
    d.src = dr->src;
    d.ess = dr->ess;
    const unsigned nblk = (unsigned)((d.S + DR_DB - 1) / DR_DB);
    const auto draw = a.hcoef ? (dr->smooth ? k_dr_draw<true, true> : k_dr_draw<false, true>)
                              : (dr->smooth ? k_dr_draw<true, false> : k_dr_draw<false, false>);
    for (size_t b0 = 0; b0 < B; b0 += DR_MAX_GRID_Y) {
        const size_t nb = (B - b0 < DR_MAX_GRID_Y) ? B - b0 : DR_MAX_GRID_Y;
        if (c || d.ess) {
            hipLaunchKernelGGL(k_dr_cdf, dim3(1, (unsigned)nb), dim3(DR_BS), 0, ctx->stream, a, b0, c, d.ess);
            ABC_HIP(ctx, hipGetLastError());
        }
        if (select) {
            hipLaunchKernelGGL(draw, dim3(nblk, (unsigned)nb), dim3(DR_BS), 0, ctx->stream, a, d, b0, sp);
            ABC_HIP(ctx, hipGetLastError());
        }
        if (a.om && c) {     // (the all-zero rule of the row weights)
            hipLaunchKernelGGL(k_dr_void, dim3((unsigned)((d.S + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream, (const double*)c,
                               K, d.S, (int)P, b0, d.draws, d.src, d.ess);
            ABC_HIP(ctx, hipGetLastError());
        }
    }
    return ABC_OK;
}
