// Box-Cox transform of the metrics (include/abcsmc_hip.h, "Box-Cox transform of the metrics"): the skewness search over a grid of
// exponents, per column, and the elementwise transform.  A pre-pass of its own: nothing here is shared with the statistics pass.
//
// The search needs the centred logs u_i = l_i - lbar of a column and, per grid value, three moments of t = exp(lambda u).  The
// skewness does not move under a positive affine map of t, so a constant added to every u_i of a column changes nothing but
// rounding: what the result is sensitive to is the DIFFERENCES of the logs.  A column of 1000 +- 0.001 has logs that agree in their
// first nine digits, and log z rounded to fp64 leaves the differences with seven.  So the logs are taken relative to the column's
// smallest entry, v_i = log1p((z_i - z_min) / z_min) = l_i - log z_min: the subtraction is exact for entries within a factor two of
// z_min and v_i keeps its relative precision however narrow the column is; u_i = v_i - vbar.  The minimum is exact in any order.
//
//   k_bc_range    grid (row blocks, columns): z_min, z_max and the validity of every column.  Positive doubles order as their bit
//                 patterns, so both are integer atomics (exact, order-free); no floating-point atomic anywhere
//   k_bc_logsum   grid (2048-row chunks, columns): the chunk's sum of v in a fixed order (8 rows per thread ascending, the wave's
//                 butterfly, the four waves ascending)
//   k_bc_mean     one wave per column: the chunks' sums in a fixed order, vbar
//   k_bc_search   grid (2048-row chunks, columns): every thread makes u for its 8 rows once, keeps them in registers and walks the
//                 L grid values: d = expm1(lambda u) (lambda == 0: d = u), the chunk's sums of d, d^2, d^3 per grid value.  N M L
//                 exponentials, 8 independent ones in flight per thread; the moments' cross-lane sums (18 shuffles per grid value
//                 and wave) are a few per cent of them.  One sweep: the sums are taken about the pilot t = 1, the image of the
//                 geometric mean, and centred at the end (k_bc_reduce).  Jensen puts the mean of t at or above 1, and for a narrow
//                 lambda u it sits lambda^2 var(u) / 2 from the pilot while the spread is |lambda| sd(u), so centring costs no
//                 digits there; for a wide lambda u the spread of t exceeds its distance from 1.  Raw sums of t would lose
//                 1 / (lambda sd(u))^3 -- everything on a narrow column.
//   k_bc_reduce   grid (32 grid values, columns): the chunks' sums in a fixed order (eight interleaved chains, then ascending), the
//                 centred moments and the skewness
//   k_bc_pick     one thread per column: the reference's ascending strict-less rule, the status bits, lambda
//   k_bc_apply    elementwise y = expm1(lambda log z) / lambda
// Every order above depends on N alone.  A column never reads another column's data, so its bits do not depend on M or on ldx.
#include <math.h>

#include "abc_internal.h"

namespace {

constexpr int BC_T = 256;                 // threads of a work-group
constexpr int BC_R = 8;                   // rows a thread keeps in registers
constexpr int BC_ROWS = BC_T * BC_R;      // rows of a chunk
constexpr int BC_W = BC_T / ABC_WAVE;     // waves of a work-group
constexpr size_t BC_MAX_GRID_Y = 65535;
constexpr int BC_RK = 32, BC_RQ = 8;      // k_bc_reduce: grid values of a work-group, interleaved chains per grid value

// per column: ~bits(z_min) and bits(z_max) (both grow under atomicMax from the zero the arena piece is cleared to), the bad flag
struct BcCol {
    unsigned long long nmin, max;
    int bad, pad;
};

__device__ inline bool bc_is_bad(const BcCol& c) { return c.bad != 0; }
__device__ inline bool bc_is_const(const BcCol& c) { return ~c.nmin == c.max; }
__device__ inline double bc_zmin(const BcCol& c) { return __longlong_as_double((long long)~c.nmin); }

// l - log z_min (above)
__device__ inline double bc_rel_log(double x, double shift, double zmin) {
    const double z = x + shift;
    return log1p((z - zmin) / zmin);
}

__device__ inline double bc_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < ABC_WAVE; m <<= 1) v += __shfl_xor(v, m, ABC_WAVE);
    return v;
}

__global__ __launch_bounds__(BC_T) void k_bc_range(const double* X, size_t ldx, size_t N, size_t M, const double* shift, BcCol* col) {
    const int t = threadIdx.x;
    for (size_t j = blockIdx.y; j < M; j += gridDim.y) {
        const double c = shift ? shift[j] : 0.0;
        const double* x = X + ldx * j;
        unsigned long long lo = ~0ull, hi = 0ull;
        int bad = 0;
        for (size_t i = (size_t)blockIdx.x * BC_T + t; i < N; i += (size_t)gridDim.x * BC_T) {
            const double z = x[i] + c;
            if (!(z > 0.0) || z == INFINITY) {
                bad = 1;
            } else {
                const unsigned long long b = (unsigned long long)__double_as_longlong(z);
                lo = b < lo ? b : lo;
                hi = b > hi ? b : hi;
            }
        }
#pragma unroll
        for (int m = 1; m < ABC_WAVE; m <<= 1) {
            const unsigned long long l2 = __shfl_xor(lo, m, ABC_WAVE), h2 = __shfl_xor(hi, m, ABC_WAVE);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
            bad |= __shfl_xor(bad, m, ABC_WAVE);
        }
        if ((t & (ABC_WAVE - 1)) == 0) {
            if (hi) {                                   // (the wave saw a valid entry)
                atomicMax(&col[j].nmin, ~lo);
                atomicMax(&col[j].max, hi);
            }
            if (bad) atomicOr(&col[j].bad, 1);
        }
    }
}

__global__ __launch_bounds__(BC_T) void k_bc_logsum(const double* X, size_t ldx, size_t N, size_t M, const double* shift, const BcCol* col,
                                                    size_t nblk, double* psum) {
    __shared__ double wsum[BC_W];
    const int t = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * BC_ROWS;
    for (size_t j = blockIdx.y; j < M; j += gridDim.y) {
        const BcCol cj = col[j];
        if (bc_is_bad(cj) || bc_is_const(cj)) continue;                     // (uniform)
        const double c = shift ? shift[j] : 0.0, zmin = bc_zmin(cj);
        const double* x = X + ldx * j;
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < BC_R; ++r) {
            const size_t i = row0 + (size_t)r * BC_T + t;
            s += i < N ? bc_rel_log(x[i], c, zmin) : 0.0;
        }
        s = bc_wave_sum(s);
        if ((t & (ABC_WAVE - 1)) == 0) wsum[t / ABC_WAVE] = s;
        __syncthreads();
        if (t == 0) {
            double a = wsum[0];
            for (int w = 1; w < BC_W; ++w) a += wsum[w];
            psum[j * nblk + blockIdx.x] = a;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(ABC_WAVE) void k_bc_mean(const BcCol* col, size_t N, size_t M, size_t nblk, const double* psum, double* mean) {
    const int t = threadIdx.x;
    for (size_t j = blockIdx.x; j < M; j += gridDim.x) {
        const BcCol cj = col[j];
        if (bc_is_bad(cj) || bc_is_const(cj)) continue;                     // (uniform)
        double s = 0.0;
        for (size_t b = t; b < nblk; b += ABC_WAVE) s += psum[j * nblk + b];
        s = bc_wave_sum(s);
        if (t == 0) mean[j] = s / (double)N;
    }
}

// part: [column][chunk][moment][grid value]
__global__ __launch_bounds__(BC_T) void k_bc_search(const double* X, size_t ldx, size_t N, size_t M, const double* shift, const BcCol* col,
                                                    const double* mean, const double* grid, int L, size_t nblk, double* part) {
    extern __shared__ double bc_sm[];                                       // [wave][moment][grid value]
    const int t = threadIdx.x, lane = t & (ABC_WAVE - 1), w = t / ABC_WAVE;
    const size_t row0 = (size_t)blockIdx.x * BC_ROWS;
    for (size_t j = blockIdx.y; j < M; j += gridDim.y) {
        const BcCol cj = col[j];
        if (bc_is_bad(cj) || bc_is_const(cj)) continue;                     // (uniform)
        const double c = shift ? shift[j] : 0.0, zmin = bc_zmin(cj), vbar = mean[j];
        const double* x = X + ldx * j;
        double u[BC_R];
#pragma unroll
        for (int r = 0; r < BC_R; ++r) {
            const size_t i = row0 + (size_t)r * BC_T + t;
            u[r] = i < N ? bc_rel_log(x[i], c, zmin) - vbar : 0.0;          // a row past the end: d = 0 for every lambda, adds nothing
        }
        for (int k = 0; k < L; ++k) {
            const double lam = grid[k];
            double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
            for (int r = 0; r < BC_R; ++r) {
                const double d = lam != 0.0 ? expm1(lam * u[r]) : u[r];
                const double d2 = d * d;
                s1 += d;
                s2 += d2;
                s3 += d2 * d;
            }
            s1 = bc_wave_sum(s1);
            s2 = bc_wave_sum(s2);
            s3 = bc_wave_sum(s3);
            if (lane == 0) {
                bc_sm[(w * 3 + 0) * L + k] = s1;
                bc_sm[(w * 3 + 1) * L + k] = s2;
                bc_sm[(w * 3 + 2) * L + k] = s3;
            }
        }
        __syncthreads();
        double* pj = part + (j * nblk + blockIdx.x) * 3 * (size_t)L;
        for (int e = t; e < 3 * L; e += BC_T) {                             // e = moment * L + grid value
            double a = bc_sm[e];
            for (int ww = 1; ww < BC_W; ++ww) a += bc_sm[ww * 3 * L + e];
            pj[e] = a;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BC_RK * BC_RQ) void k_bc_reduce(const BcCol* col, size_t N, size_t M, const double* grid, int L, size_t nblk,
                                                             const double* part, double* skew, double* skew_out) {
    __shared__ double sm[3][BC_RQ][BC_RK];
    const int t = threadIdx.x, kk = t % BC_RK, q = t / BC_RK;
    const int k = (int)blockIdx.x * BC_RK + kk;
    for (size_t j = blockIdx.y; j < M; j += gridDim.y) {
        const BcCol cj = col[j];
        const bool bad = bc_is_bad(cj), flat = bc_is_const(cj);
        if (bad || flat) {                                                  // (uniform)
            if (q == 0 && k < L) {
                const double v = bad ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
                skew[j * L + k] = v;
                if (skew_out) skew_out[j * L + k] = v;
            }
            continue;
        }
        double s[3] = {0.0, 0.0, 0.0};
        if (k < L)
            for (size_t b = q; b < nblk; b += BC_RQ) {
                const double* pb = part + (j * nblk + b) * 3 * (size_t)L + k;
                s[0] += pb[0];
                s[1] += pb[L];
                s[2] += pb[2 * (size_t)L];
            }
        sm[0][q][kk] = s[0];
        sm[1][q][kk] = s[1];
        sm[2][q][kk] = s[2];
        __syncthreads();
        if (q == 0 && k < L) {
            double S1 = sm[0][0][kk], S2 = sm[1][0][kk], S3 = sm[2][0][kk];
            for (int qq = 1; qq < BC_RQ; ++qq) {
                S1 += sm[0][qq][kk];
                S2 += sm[1][qq][kk];
                S3 += sm[2][qq][kk];
            }
            // sums about the pilot -> centred sums: m = mean of d; sum (d - m)^2 = S2 - m S1; sum (d - m)^3 = S3 - 3 m S2 + 2 m^2 S1
            const double n = (double)N, m = S1 / n;
            const double c2 = S2 - m * S1;
            const double c3 = (S3 - 3.0 * m * S2) + 2.0 * (m * m) * S1;
            const double var = c2 / (n - 1.0);
            const double sk = (c3 / n) / (var * sqrt(var));
            const double v = grid[k] < 0.0 ? -sk : sk;
            skew[j * L + k] = v;
            if (skew_out) skew_out[j * L + k] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BC_T) void k_bc_pick(const BcCol* col, size_t M, const double* grid, int L, const double* skew, double* lambda,
                                                  double* best_skew, int32_t* pick, int32_t* status) {
    const size_t j = (size_t)blockIdx.x * BC_T + threadIdx.x;
    if (j >= M) return;
    const BcCol cj = col[j];
    const double* sj = skew + j * L;
    int st = 0, pk = 0;
    double lam = 1.0;
    if (bc_is_bad(cj)) {
        st = 1;
        pk = -1;
    } else {
        if (bc_is_const(cj)) st = 2;
        double best = INFINITY;
        for (int k = 0; k < L; ++k) {
            const double s = sj[k];
            if (!isfinite(s)) { st |= 4; continue; }
            if (fabs(s) < fabs(best)) { best = s; pk = k; }
        }
        lam = grid[pk];
    }
    lambda[j] = lam;
    if (best_skew) best_skew[j] = sj[pk < 0 ? 0 : pk];
    if (pick) pick[j] = pk;
    if (status) status[j] = st;
}

__global__ __launch_bounds__(BC_T) void k_bc_apply(const double* X, size_t ldx, size_t n, size_t M, const double* lambda, const double* shift,
                                                   double* out, size_t ldo) {
    const int t = threadIdx.x;
    for (size_t j = blockIdx.y; j < M; j += gridDim.y) {
        const double lam = lambda[j], c = shift ? shift[j] : 0.0;
        const double* x = X + ldx * j;
        double* o = out + ldo * j;
        for (size_t i = (size_t)blockIdx.x * BC_T + t; i < n; i += (size_t)gridDim.x * BC_T) {
            const double l = log(x[i] + c);
            o[i] = lam != 0.0 ? expm1(lam * l) / lam : l;
        }
    }
}

inline size_t bc_chunks(size_t N) { return (N + BC_ROWS - 1) / BC_ROWS; }

}  // namespace

size_t abc_box_cox_need(size_t N, size_t M, size_t L) {
    const size_t nblk = bc_chunks(N);
    return abc_align(M * sizeof(BcCol), 256) + abc_align(M * nblk * 8, 256) + abc_align(M * 8, 256) +
           abc_align(M * nblk * 3 * L * 8, 256) + abc_align(M * L * 8, 256) + 2048;
}

int launch_box_cox_search(abc_ctx* ctx, const double* X, size_t ldx, size_t N, size_t M, const double* shift, const double* grid, size_t L,
                          const abc_box_cox_out* out) {
    const size_t nblk = bc_chunks(N);
    BcCol* col = (BcCol*)abc_ws_alloc(ctx, M * sizeof(BcCol));
    double* psum = (double*)abc_ws_alloc(ctx, M * nblk * 8);
    double* mean = (double*)abc_ws_alloc(ctx, M * 8);
    double* part = (double*)abc_ws_alloc(ctx, M * nblk * 3 * L * 8);
    double* skew = (double*)abc_ws_alloc(ctx, M * L * 8);
    if (!col || !psum || !mean || !part || !skew) return ABC_ERR_NOMEM;
    const unsigned gy = (unsigned)(M < BC_MAX_GRID_Y ? M : BC_MAX_GRID_Y);
    size_t rb = (N + BC_T - 1) / BC_T;
    if (rb > 1024) rb = 1024;
    ABC_HIP(ctx, hipMemsetAsync(col, 0, M * sizeof(BcCol), ctx->stream));
    hipLaunchKernelGGL(k_bc_range, dim3((unsigned)rb, gy), dim3(BC_T), 0, ctx->stream, X, ldx, N, M, shift, col);
    ABC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bc_logsum, dim3((unsigned)nblk, gy), dim3(BC_T), 0, ctx->stream, X, ldx, N, M, shift, (const BcCol*)col, nblk, psum);
    ABC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bc_mean, dim3(gy), dim3(ABC_WAVE), 0, ctx->stream, (const BcCol*)col, N, M, nblk, (const double*)psum, mean);
    ABC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bc_search, dim3((unsigned)nblk, gy), dim3(BC_T), BC_W * 3 * L * sizeof(double), ctx->stream, X, ldx, N, M, shift,
                       (const BcCol*)col, (const double*)mean, grid, (int)L, nblk, part);
    ABC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bc_reduce, dim3((unsigned)((L + BC_RK - 1) / BC_RK), gy), dim3(BC_RK * BC_RQ), 0, ctx->stream, (const BcCol*)col, N, M,
                       grid, (int)L, nblk, (const double*)part, skew, out->skew);
    ABC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bc_pick, dim3((unsigned)((M + BC_T - 1) / BC_T)), dim3(BC_T), 0, ctx->stream, (const BcCol*)col, M, grid, (int)L,
                       (const double*)skew, out->lambda, out->best_skew, out->pick, out->status);
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}

int launch_box_cox_apply(abc_ctx* ctx, const double* X, size_t ldx, size_t n, size_t M, const double* lambda, const double* shift, double* out,
                         size_t ldo) {
    size_t rb = (n + BC_T - 1) / BC_T;
    if (rb > 4096) rb = 4096;
    const unsigned gy = (unsigned)(M < BC_MAX_GRID_Y ? M : BC_MAX_GRID_Y);
    hipLaunchKernelGGL(k_bc_apply, dim3((unsigned)rb, gy), dim3(BC_T), 0, ctx->stream, X, ldx, n, M, lambda, shift, out, ldo);
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}
