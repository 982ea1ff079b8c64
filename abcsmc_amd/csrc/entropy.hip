// Posterior entropy of segments (abc_rank_targets_entropy_dev, abc_weighted_entropy_dev; the definition is in the header): the
// Kozachenko-Leonenko k-nearest-neighbour estimate over a target's K entries in all P parameters at once.  The values of (target b,
// parameter j) are made by segment_dev.h, as every other product's; the entries' weights are all equal by the entries' refusals.
//   k_en_values  writes the targets' scaled values u_e[j] = v_e[j] / scale[j] once into the workspace, row-major [b][e][j], one
//                thread per (e, j); a non-finite u raises the target's flag (a plain store of 1: every writer stores the same word).
//   k_en_knn     the hot path, P <= EN_PREG.  Grid (tiles of EN_BS rows, targets), one thread per row e.  The thread's own values sit
//                in PW registers (PW: P rounded up to 1, 2, 4, 8, 16; the pad is 0 on both sides, and fma(0, 0, acc) == acc, so the
//                chain keeps its bits).  The target's rows pass through LDS in chunks of EN_CH rows (EN_CH PW doubles: 32 KiB at
//                PW = 16, so four work-groups fit on a CU); every lane reads the same row f at a time, a broadcast read.  d2(e, f) is
//                the definition's fma chain, j ascending.  The k smallest distances are kept sorted in k registers; k is a template
//                argument (KN), not eight fixed slots: the slots' 16 registers would cost no occupancy, but the insertion's
//                instructions are what costs, and eight slots double them at the usual k = 4; rho2 is then slot k - 1 at a constant
//                index, so nothing goes to scratch.  A distance enters by a compare-and-select chain that a wave skips when none
//                of its lanes has a candidate.
//   k_en_knn_wide  P > EN_PREG.  The same grid and thread.  The own rows no longer fit in registers, so they are read from LDS: a
//                slice of EN_JS parameters of the tile's rows, laid out [j][e] (row stride EN_BS + 1: the staging stores and the
//                loop's loads are both conflict-free).  A pair's chain has to run over all slices before it ends, so the thread
//                keeps EN_FG accumulators, one per row f of a group whose slice is staged beside the own one (broadcast reads), and
//                the slices are the inner loop.  The own slices are staged once per group: K / EN_FG times the tile's bytes come from
//                L2.  This is the instance for completeness (P up to 1024), not the one the measurements are about.
//   k_en_reduce  one work-group per target: a thread sums log rho2_e over e = t, t + 256, ... ascending, then a fixed tree over the
//                threads: an order that depends on K only.  It counts the zeros, writes knn = sqrt(rho2) and H = c + coef sum.
// No floating-point atomics; a target's outputs depend on its own segment only, and not on the members asked for: rho2 always goes
// to the workspace.
#include <math.h>

#include "abc_internal.h"
#include "segment_dev.h"

namespace {

constexpr int EN_BS = 256;                                  // threads of every work-group: the rows of a tile
constexpr int EN_CH = 256;                                  // rows of a staged chunk (k_en_knn)
constexpr int EN_PREG = 16;                                 // widest P whose own values stay in registers
constexpr int EN_JS = 16;                                   // parameters of a slice (k_en_knn_wide)
constexpr int EN_FG = 16;                                   // rows f of a group, one accumulator each (k_en_knn_wide)
constexpr unsigned EN_MAX_GRID_Y = 65535;
static_assert(EN_CH * EN_PREG * 8 <= 65536, "the staged chunk stays at or below 64 KiB");
static_assert(EN_BS % EN_JS == 0 && (EN_FG * EN_JS) <= EN_BS, "the staging loops of k_en_knn_wide");

__device__ __forceinline__ double en_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double en_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// d enters the KN smallest, kept ascending (no NaN reaches this: the values are finite or the target is flagged)
template <int KN>
__device__ __forceinline__ void en_insert(double (&best)[KN], double d) {
    if (d < best[KN - 1]) {
#pragma unroll
        for (int s = 0; s < KN; s++) {
            const bool lt = d < best[s];
            const double lo = lt ? d : best[s];
            d = lt ? best[s] : d;
            best[s] = lo;
        }
    }
}

// grid (blocks of 256 of the target's K P values, targets b0 + blockIdx.y); scale: P values (device) or NULL
template <bool TF, bool HC>
__global__ __launch_bounds__(256) void k_en_values(SmArgs a, size_t b0, const double* __restrict__ scale, double* __restrict__ U,
                                                   unsigned* __restrict__ bad) {
    const size_t b = b0 + blockIdx.y, P = (size_t)a.P, n = a.K * P;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t e = i / P;
    const int j = (int)(i - e * P);
    SmSeg s = sm_seg(a, b, 0);                                  // sm_seg(a, b, j): the members that depend on j
    s.j = j;
    if (a.method == 1) s.beta += j;
    if constexpr (HC) sm_seg_hc(a, s);
    double v = sm_value<TF, HC>(a, s, e);
    if (scale) v = v / scale[j];
    U[b * n + i] = v;
    if (!(fabs(v) < en_inf())) bad[b] = 1u;
}

// grid (tiles of EN_BS rows, targets b0 + blockIdx.y); P <= PW
template <int PW, int KN>
__global__ __launch_bounds__(EN_BS) void k_en_knn(const double* __restrict__ U, size_t K, int P, size_t b0,
                                                  double* __restrict__ rho2) {
    __shared__ double ch[EN_CH * PW];
    const int t = threadIdx.x;
    const size_t b = b0 + blockIdx.y, e = (size_t)blockIdx.x * EN_BS + t;
    const double* __restrict__ Ub = U + b * K * (size_t)P;
    double x[PW], best[KN];
#pragma unroll
    for (int j = 0; j < PW; j++) x[j] = (j < P && e < K) ? Ub[e * (size_t)P + j] : 0.0;
#pragma unroll
    for (int s = 0; s < KN; s++) best[s] = en_inf();
    if (P < PW)                                                 // (the pad: no chunk overwrites it)
        for (int i = t; i < EN_CH * PW; i += EN_BS) ch[i] = 0.0;
    for (size_t f0 = 0; f0 < K; f0 += EN_CH) {
        const int nr = (K - f0 < (size_t)EN_CH) ? (int)(K - f0) : EN_CH;
        __syncthreads();
        for (int i = t; i < nr * P; i += EN_BS) {
            const int r = i / P;
            ch[r * PW + (i - r * P)] = Ub[f0 * (size_t)P + i];
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < nr; r++) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < PW; j++) {
                const double dl = x[j] - ch[r * PW + j];
                acc = fma(dl, dl, acc);
            }
            if (f0 + (size_t)r != e) en_insert<KN>(best, acc);
        }
    }
    if (e < K) rho2[b * K + e] = best[KN - 1];
}

// grid (tiles of EN_BS rows, targets b0 + blockIdx.y); any P
template <int KN>
__global__ __launch_bounds__(EN_BS) void k_en_knn_wide(const double* __restrict__ U, size_t K, int P, size_t b0,
                                                       double* __restrict__ rho2) {
    __shared__ double own[EN_JS * (EN_BS + 1)];
    __shared__ double oth[EN_FG * EN_JS];
    const int t = threadIdx.x;
    const size_t b = b0 + blockIdx.y, e0 = (size_t)blockIdx.x * EN_BS, e = e0 + t;
    const double* __restrict__ Ub = U + b * K * (size_t)P;
    double best[KN];
#pragma unroll
    for (int s = 0; s < KN; s++) best[s] = en_inf();
    for (size_t g0 = 0; g0 < K; g0 += EN_FG) {
        double acc[EN_FG];
#pragma unroll
        for (int q = 0; q < EN_FG; q++) acc[q] = 0.0;
        for (int j0 = 0; j0 < P; j0 += EN_JS) {
            __syncthreads();
            for (int i = t; i < EN_BS * EN_JS; i += EN_BS) {   // own[j][row]: 0 past K and past P
                const int r = i / EN_JS, j = i - r * EN_JS;
                own[j * (EN_BS + 1) + r] = (e0 + r < K && j0 + j < P) ? Ub[(e0 + r) * (size_t)P + j0 + j] : 0.0;
            }
            if (t < EN_FG * EN_JS) {                            // oth[q][j]
                const int q = t / EN_JS, j = t - q * EN_JS;
                oth[t] = (g0 + q < K && j0 + j < P) ? Ub[(g0 + q) * (size_t)P + j0 + j] : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int j = 0; j < EN_JS; j++) {
                const double xj = own[j * (EN_BS + 1) + t];
#pragma unroll
                for (int q = 0; q < EN_FG; q++) {
                    const double dl = xj - oth[q * EN_JS + j];
                    acc[q] = fma(dl, dl, acc[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < EN_FG; q++)
            if (g0 + q < K && g0 + q != e) en_insert<KN>(best, acc[q]);
    }
    if (e < K) rho2[b * K + e] = best[KN - 1];
}

struct EnOut {
    double* H;
    double* knn;
    uint64_t* zeros;
};

// grid (1, targets b0 + blockIdx.y); few: K <= k, nothing was computed and every output is the rule's
__global__ __launch_bounds__(256) void k_en_reduce(const double* __restrict__ rho2, const unsigned* __restrict__ bad, size_t K,
                                                   size_t b0, double c, double coef, int few, EnOut o) {
    __shared__ double ss[256];
    __shared__ unsigned long long sz[256];
    const int t = threadIdx.x;
    const size_t b = b0 + blockIdx.y;
    const bool nan = few || bad[b] != 0u;
    double s = 0.0;
    unsigned long long z = 0;
    for (size_t e = t; e < K; e += 256) {
        const double r = nan ? en_nan() : rho2[b * K + e];
        s += log(r);
        z += (r == 0.0) ? 1u : 0u;
        if (o.knn) o.knn[b * K + e] = nan ? en_nan() : sqrt(r);
    }
    ss[t] = s;
    sz[t] = z;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) {
            ss[t] += ss[t + st];
            sz[t] += sz[t + st];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (o.H) o.H[b] = nan ? en_nan() : sz[0] ? -en_inf() : c + coef * ss[0];
        if (o.zeros) o.zeros[b] = nan ? 0 : (uint64_t)sz[0];
    }
}

typedef void (*EnKnn)(const double*, size_t, int, size_t, double*);

// the instance for k = 1..8: F<KN>::fn
template <template <int> class F>
EnKnn en_by_k(int k) {
    static const EnKnn tab[8] = {F<1>::fn, F<2>::fn, F<3>::fn, F<4>::fn, F<5>::fn, F<6>::fn, F<7>::fn, F<8>::fn};
    return tab[k - 1];
}
template <int PW>
struct EnReg {
    template <int KN>
    struct At { static constexpr EnKnn fn = k_en_knn<PW, KN>; };
};
template <int KN>
struct EnWide { static constexpr EnKnn fn = k_en_knn_wide<KN>; };

}  // namespace

size_t abc_entropy_need(size_t B, size_t K, size_t P) {
    return B * K * P * 8 + B * K * 8 + P * 8 + B * 4 + 8 * 256;   // the scaled values, rho2, scale, the flags
}

int launch_entropy(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const abc_entropy* en, const char* fn) {
    if (B == 0 || K == 0 || P == 0) return ABC_OK;
    const int k = en->k;
    const bool few = K <= (size_t)k;
    // c = (P / 2) log pi - lgamma(P / 2 + 1) - psi(k) + log n, psi(k) = -gamma + sum_{m < k} 1 / m (m ascending), in double
    double psi = 0.0;
    for (int m = 1; m < k; m++) psi += 1.0 / (double)m;
    psi -= 0.57721566490153286061;
    const double hp = 0.5 * (double)P;
    const double c = hp * std::log(3.14159265358979323846) - std::lgamma(hp + 1.0) - psi + std::log((double)K);
    const double coef = (double)P / (2.0 * (double)K);
    const EnOut o = {en->H, en->knn, en->zeros};
    double* U = nullptr;
    double* rho2 = nullptr;
    double* scale = nullptr;
    unsigned* bad = nullptr;
    if (!few) {
        U = (double*)abc_ws_alloc(ctx, B * K * P * 8);
        rho2 = (double*)abc_ws_alloc(ctx, B * K * 8);
        bad = (unsigned*)abc_ws_alloc(ctx, B * 4);
        if (en->scale) scale = (double*)abc_ws_alloc(ctx, P * 8);
        if (!U || !rho2 || !bad || (en->scale && !scale)) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
        if (scale) ABC_HIP(ctx, hipMemcpyAsync(scale, en->scale, P * 8, hipMemcpyHostToDevice, ctx->stream));
        ABC_HIP(ctx, hipMemsetAsync(bad, 0, B * 4, ctx->stream));
    }
    const SmArgs a = sm_args(sv, K, P);
    const auto values = a.hcoef ? k_en_values<true, true> : a.tf.kind ? k_en_values<true, false> : k_en_values<false, false>;
    const EnKnn knn = P > (size_t)EN_PREG ? en_by_k<EnWide>(k)
                      : P > 8 ? en_by_k<EnReg<16>::At>(k)
                      : P > 4 ? en_by_k<EnReg<8>::At>(k)
                      : P > 2 ? en_by_k<EnReg<4>::At>(k)
                      : P > 1 ? en_by_k<EnReg<2>::At>(k)
                              : en_by_k<EnReg<1>::At>(k);
    if ((K * P + 255) / 256 > 0x7fffffffu) ABC_FAIL(ctx, ABC_ERR_UNSUPPORTED, "%s: K P = %zu values of a target (below 2^39)", fn, K * P);
    const unsigned nval = (unsigned)((K * P + 255) / 256), ntile = (unsigned)((K + EN_BS - 1) / EN_BS);
    for (size_t b0 = 0; b0 < B; b0 += EN_MAX_GRID_Y) {
        const unsigned nb = (unsigned)((B - b0 < EN_MAX_GRID_Y) ? B - b0 : EN_MAX_GRID_Y);
        if (!few) {
            hipLaunchKernelGGL(values, dim3(nval, nb), dim3(256), 0, ctx->stream, a, b0, (const double*)scale, U, bad);
            ABC_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(knn, dim3(ntile, nb), dim3(EN_BS), 0, ctx->stream, (const double*)U, K, (int)P, b0, rho2);
            ABC_HIP(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(k_en_reduce, dim3(1, nb), dim3(256), 0, ctx->stream, (const double*)rho2, (const unsigned*)bad, K, b0, c, coef,
                           few ? 1 : 0, o);
        ABC_HIP(ctx, hipGetLastError());
    }
    return ABC_OK;
}
