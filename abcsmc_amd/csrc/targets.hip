// Batched PLS ranking: one fitted model, one set of rows, B observed targets (abc_rank_targets_dev).
//
// Target b's result is, bit for bit, the first K entries of the single-target ranking with obs = targets[b]: ascending
// (dist, row), dist = sqrt of the fma chain over components k < ncomp of (s_k - o_k)^2.  Nothing before the target scores
// depends on the observation, so the work is:
//   k_tg_scores     the B x A target scores: z = (t - mean) / sd (0 where sd == 0), o_k = m-ascending fma chain against R --
//                   the fit's own formula for the observed scores (pls.hip)
//   scores of every row, once: launch_project_distance_scores with row_test = 0 (the projection kernels' chains), or
//                   k_tg_row_scores where its conditions do not hold (same chains)
//   k_tg_sample     the scores of up to 4096 evenly spaced rows, gathered once for all targets
//   k_tg_threshold  one work-group per target: the sample's distances, sorted in LDS; the key of sample rank
//                   K/N * 4096 + 4 sigma + 8 (all rows, exact K-th: small sets) is the target's threshold
//   k_tg_cand       THE pass over the scores: a work-group holds 256 x 1..4 rows' scores in registers and walks the targets (their
//                   scores read through the scalar cache); a squared distance below a conservative bound of the threshold
//                   is rooted, and rows whose exact key is at or below it go to the target's candidate segment with one
//                   atomic per wave
//   k_tg_bins       one work-group per target: linear bins over the candidates' key range, the bin of the K-th key, a
//                   scatter of the candidates of the bins up to it (the sampled-range selection of select.hip, per segment)
//   k_tg_sort       bitonic sort of every bin by (key, row) in LDS, written to the target's output
// A target whose segment overflowed, held fewer than K candidates, or had a bin too large for LDS is flagged and recomputed
// by the exact single-target path (its distances from the scores, launch_select_smallest).
#include <math.h>

#include <vector>

#include "abc_internal.h"
#include "project_plan.h"

namespace {

constexpr int TG_S = 4096;      // sampled rows
constexpr int TG_NB = 2048;     // linear bins per target
constexpr int TG_CAP = 1024;    // keys one work-group sorts

__device__ __forceinline__ unsigned long long tg_key(double d) {      // order-preserving key (select.hip's key_of)
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double tg_dist(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ int tg_ncomp(const double* model, int A) {
    const int nc = (int)model[0];
    return nc < 0 ? 0 : (nc > A ? A : nc);
}

__device__ __forceinline__ int tg_bin(unsigned long long k, unsigned long long lo, int shift) {
    return (k <= lo) ? 0 : (int)((k - lo) >> shift);
}

struct TgInfo {
    unsigned long long tkey;    // threshold key (candidates: key <= tkey)
    double t2;                  // conservative bound of the squared distance at the threshold
    unsigned long long lo;      // bin range [lo, tkey]: the sample's smallest key
    int shift, bstar;
    unsigned int need, pad_;
};

// O[b * KC + k] = score k of target b for k < ncomp, 0 beyond (KC >= A)
__global__ __launch_bounds__(256) void k_tg_scores(const double* __restrict__ T, size_t ldt, size_t B, int M, int A, int KC,
                                                   const double* __restrict__ model, size_t off_mean, size_t off_sd, size_t off_R,
                                                   double* __restrict__ O, int* __restrict__ bad) {
    const int nc = tg_ncomp(model, A);
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * (size_t)KC) return;
    const size_t b = e / KC;
    const int k = (int)(e % KC);
    if (k == 0)
        for (int m = 0; m < M; m++)
            if (!isfinite(T[b + ldt * m])) atomicOr(bad, 1);
    double s = 0.0;
    if (k < nc)
        for (int m = 0; m < M; m++) {
            const double sdv = model[off_sd + m];
            const double z = (sdv == 0.0) ? 0.0 : (T[b + ldt * m] - model[off_mean + m]) / sdv;
            s = fma(z, model[off_R + m + (size_t)M * k], s);
        }
    O[e] = s;
}

// S[i + sld k] = score k of row i (all A components), the projection kernels' chain: for m ascending, z = (x - mean) / sd,
// s_k = fma(z, R[m, k], s_k).  Eight components per sweep over the row's metrics.
__global__ __launch_bounds__(256) void k_tg_row_scores(const double* __restrict__ X, size_t n, size_t ldx, int M, int A,
                                                       const double* __restrict__ model, size_t off_mean, size_t off_sd, size_t off_R,
                                                       double* __restrict__ S, size_t sld) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const double* xp = X + i;
        for (int c0 = 0; c0 < A; c0 += 8) {
            double s[8];
#pragma unroll
            for (int u = 0; u < 8; u++) s[u] = 0.0;
            for (int m = 0; m < M; m++) {
                const double sdv = model[off_sd + m];
                const double z = (sdv == 0.0) ? 0.0 : (xp[(size_t)m * ldx] - model[off_mean + m]) / sdv;
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (c0 + u < A) s[u] = fma(z, model[off_R + m + (size_t)M * (c0 + u)], s[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (c0 + u < A) S[i + sld * (size_t)(c0 + u)] = s[u];
        }
    }
}

__device__ __forceinline__ size_t tg_sample_row(int j, size_t n, int ns) {
    if ((size_t)ns == n) return (size_t)j;
    const size_t stride = n / (size_t)ns;
    return (size_t)j * stride + stride / 2;
}

// Ss[j * KC + k] = score k of sampled row j (0 for k >= ncomp)
__global__ __launch_bounds__(256) void k_tg_sample(const double* __restrict__ S, size_t n, size_t sld, int ns, int A, int KC,
                                                   const double* __restrict__ model, double* __restrict__ Ss) {
    const int nc = tg_ncomp(model, A);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ns * KC) return;
    const int j = e / KC, k = e % KC;
    Ss[e] = (k < nc) ? S[tg_sample_row(j, n, ns) + sld * (size_t)k] : 0.0;
}

// one work-group per target: the sample's keys, bitonic-sorted in LDS; the key of rank q is the threshold
__global__ __launch_bounds__(1024) void k_tg_threshold(const double* __restrict__ Ss, size_t n, int ns, int q, int KC,
                                                       const double* __restrict__ O, const unsigned long long* __restrict__ excl,
                                                       TgInfo* __restrict__ info) {
    __shared__ unsigned long long sk[TG_S];
    const int t = threadIdx.x;
    const size_t b = blockIdx.x;
    const double* o = O + b * KC;
    const unsigned long long ex = excl ? excl[b] : ~0ull;
    for (int j = t; j < TG_S; j += 1024) {
        unsigned long long key = ~0ull;
        if (j < ns && tg_sample_row(j, n, ns) != ex) {
            double d2 = 0.0;
            for (int k = 0; k < KC; k++) { const double d = Ss[(size_t)j * KC + k] - o[k]; d2 = fma(d, d, d2); }
            key = tg_key(sqrt(d2));
        }
        sk[j] = key;
    }
    __syncthreads();
    for (int k = 2; k <= TG_S; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < TG_S / 2; p += 1024) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const unsigned long long a = sk[i], c = sk[i + j];
                if ((a > c) == ((i & k) == 0)) { sk[i] = c; sk[i + j] = a; }
            }
            __syncthreads();
        }
    if (t == 0) {
        const unsigned long long T = sk[q];
        double t2;
        if (T >= tg_key(INFINITY)) t2 = INFINITY;                       // +inf or a positive NaN: every finite distance
        else if (T < tg_key(0.0)) t2 = -1.0;                            // below +0 (a negative NaN): only NaN rows can be candidates
        else {
            // sqrt(d2) <= td implies d2 < u^2 with u the next double above td; two steps up from the rounded square cover u^2
            const double u = nextafter(tg_dist(T), INFINITY);
            t2 = nextafter(nextafter(u * u, INFINITY), INFINITY);
        }
        info[b].tkey = T;
        info[b].t2 = t2;
        info[b].lo = sk[0];
    }
}

// The candidate pass.  blockIdx.x: 256 RPT rows (RPT per thread, 256 apart); blockIdx.y: a group of targets [b0, b1).  KC: the
// padded component count held in registers (1..32); KC == 0: more than 32 components, read from the scores as they are needed.
// A wave takes ONE atomic per target for all its RPT x 64 rows; the counters sit 128 bytes apart (TG_CSTRIDE): packed on one
// cache line, the targets' atomics serialise on one L2 channel.
constexpr int TG_CSTRIDE = 32;
template <int KC, int RPT>
__global__ __launch_bounds__(256) void k_tg_cand(const double* __restrict__ S, size_t n, size_t sld, int A, int KCO,
                                                 const double* __restrict__ model, const double* __restrict__ O, size_t B,
                                                 size_t tgs, const unsigned long long* __restrict__ excl,
                                                 const TgInfo* __restrict__ info, size_t C, unsigned int* __restrict__ cnt,
                                                 unsigned long long* __restrict__ ckey, unsigned int* __restrict__ crow) {
    constexpr int KR = KC > 0 ? KC : 1;
    const int nc = tg_ncomp(model, A);
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    size_t row[RPT];
    bool valid[RPT];
    double s[RPT][KR];
#pragma unroll
    for (int r = 0; r < RPT; r++) {
        row[r] = (size_t)blockIdx.x * 256 * RPT + (size_t)r * 256 + threadIdx.x;
        valid[r] = row[r] < n;
#pragma unroll
        for (int k = 0; k < KR; k++) s[r][k] = (KC > 0 && valid[r] && k < nc) ? S[row[r] + sld * (size_t)k] : 0.0;
    }
    const size_t b0 = (size_t)blockIdx.y * tgs, b1 = (b0 + tgs < B) ? b0 + tgs : B;
    for (size_t b = b0; b < b1; b++) {
        const double* o = O + b * KCO;
        const double t2 = info[b].t2;
        const unsigned long long tkey = info[b].tkey, ex = excl ? excl[b] : ~0ull;
        double d2[RPT];
        bool pass[RPT];
        unsigned long long any = 0ull;
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            d2[r] = 0.0;
            if (KC > 0) {
#pragma unroll
                for (int k = 0; k < KR; k++) { const double d = s[r][k] - o[k]; d2[r] = fma(d, d, d2[r]); }
            } else {
                for (int k = 0; k < nc; k++) {
                    const double d = (valid[r] ? S[row[r] + sld * (size_t)k] : 0.0) - o[k];
                    d2[r] = fma(d, d, d2[r]);
                }
            }
            pass[r] = valid[r] && (d2[r] <= t2 || d2[r] != d2[r]) && row[r] != ex;
            any |= __ballot(pass[r]);
        }
        if (any == 0ull) continue;
        unsigned long long mask[RPT];
        unsigned long long key[RPT];
        unsigned int tot = 0;
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            key[r] = 0;
            mask[r] = 0ull;
            if (__ballot(pass[r]) == 0ull) continue;
            key[r] = tg_key(sqrt(d2[r]));
            pass[r] = pass[r] && key[r] <= tkey;
            mask[r] = __ballot(pass[r]);
            tot += (unsigned int)__popcll(mask[r]);
        }
        if (tot == 0) continue;
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(&cnt[b * TG_CSTRIDE], tot);
        base = __shfl(base, 0, 64);
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            if (pass[r]) {
                const size_t p = (size_t)base + (size_t)__popcll(mask[r] & lt);
                if (p < C) { ckey[b * C + p] = key[r]; crow[b * C + p] = (unsigned int)row[r]; }
            }
            base += (unsigned int)__popcll(mask[r]);
        }
    }
}

// one work-group per target of the chunk: bins of the candidates, the bin of the K-th key, scatter of the bins up to it
__global__ __launch_bounds__(1024) void k_tg_bins(const unsigned int* __restrict__ cnt, size_t C, unsigned long long K,
                                                  TgInfo* __restrict__ info, int* __restrict__ fail,
                                                  const unsigned long long* __restrict__ ckey, const unsigned int* __restrict__ crow,
                                                  unsigned int* __restrict__ offs, unsigned long long* __restrict__ skey,
                                                  unsigned int* __restrict__ srow) {
    __shared__ unsigned int h[TG_NB + 1];
    __shared__ int s_fail;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t b = blockIdx.x;
    const unsigned int c = cnt[b * TG_CSTRIDE];
    if ((size_t)c > C || (unsigned long long)c < K) { if (t == 0) fail[b] = 1; return; }
    const unsigned long long* kk = ckey + b * C;
    const unsigned int* rr = crow + b * C;
    for (int e = t; e <= TG_NB; e += 1024) h[e] = 0;
    if (t == 0) s_fail = 0;
    __syncthreads();
    // bins from the sample's smallest key (a zero-distance row does not stretch the range: it goes to bin 0)
    // (extended below it by the span up to the threshold: the rows under the sample's minimum spread over bins of their own)
    const unsigned long long lo0 = info[b].lo, hi = info[b].tkey, k0 = tg_key(0.0);
    const unsigned long long span = hi - lo0, room = (lo0 > k0) ? lo0 - k0 : 0ull;
    const unsigned long long lo = lo0 - (span < room ? span : room);
    int shift = 0;
    while (shift < 63 && ((hi - lo) >> shift) >= (unsigned long long)(TG_NB - 1)) shift++;
    for (unsigned int e = t; e < c; e += 1024) atomicAdd(&h[tg_bin(kk[e], lo, shift)], 1u);
    __syncthreads();
    // exclusive scan of the bins (two per thread) -> offsets; the bin of the K-th key
    __shared__ unsigned int wsum[16];
    __shared__ int s_bstar;
    __shared__ unsigned int s_need;
    const unsigned int c0 = h[2 * t], c1 = h[2 * t + 1], sum = c0 + c1;
    unsigned int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned int u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned int run = inc - sum;
    for (int w = 0; w < wave; w++) run += wsum[w];
    const unsigned int off0 = run, off1 = run + c0;
    if ((unsigned long long)off0 < K && K <= (unsigned long long)off0 + c0) { s_bstar = 2 * t; s_need = (unsigned int)(K - off0); }
    if ((unsigned long long)off1 < K && K <= (unsigned long long)off1 + c1) { s_bstar = 2 * t + 1; s_need = (unsigned int)(K - off1); }
    if (((unsigned long long)off0 < K && c0 > (unsigned int)TG_CAP) || ((unsigned long long)off1 < K && c1 > (unsigned int)TG_CAP)) s_fail = 1;
    __syncthreads();
    unsigned int* of = offs + b * (TG_NB + 1);
    of[2 * t] = off0;
    of[2 * t + 1] = off1;
    if (t == 0) of[TG_NB] = c;
    if (s_fail) { if (t == 0) fail[b] = 1; return; }
    const int bstar = s_bstar;
    if (t == 0) { info[b].shift = shift; info[b].bstar = bstar; info[b].need = s_need; }
    h[2 * t] = off0;                                    // the bins' cursors
    h[2 * t + 1] = off1;
    __syncthreads();
    for (unsigned int e = t; e < c; e += 1024) {
        const unsigned long long v = kk[e];
        const int bin = tg_bin(v, lo, shift);
        if (bin > bstar) continue;
        const unsigned int p = atomicAdd(&h[bin], 1u);
        skey[b * C + p] = v;
        srow[b * C + p] = rr[e];
    }
}

// bins [blockIdx.x, b*] step gridDim.x of target blockIdx.y: bitonic sort by (key, row), the kept part to the output
__global__ __launch_bounds__(256) void k_tg_sort(const TgInfo* __restrict__ info, const int* __restrict__ fail,
                                                 const unsigned int* __restrict__ offs, const unsigned long long* __restrict__ skey,
                                                 const unsigned int* __restrict__ srow, size_t C, unsigned long long K,
                                                 uint64_t* __restrict__ idx, double* __restrict__ dist) {
    __shared__ unsigned long long sk[TG_CAP];
    __shared__ unsigned int si[TG_CAP];
    const size_t b = blockIdx.y;
    const int t = threadIdx.x;
    if (fail[b]) return;
    const int bstar = info[b].bstar;
    const unsigned int need = info[b].need;
    const unsigned int* of = offs + b * (TG_NB + 1);
    for (int bin = blockIdx.x; bin <= bstar; bin += gridDim.x) {
        const unsigned int o0 = of[bin], cnt = of[bin + 1] - o0;
        if (cnt == 0) continue;                                      // (uniform)
        const unsigned int keep = (bin == bstar) ? need : cnt;
        unsigned int n2 = 1;
        while (n2 < cnt) n2 <<= 1;
        __syncthreads();
        for (unsigned int e = t; e < n2; e += 256) {
            sk[e] = (e < cnt) ? skey[b * C + o0 + e] : ~0ull;
            si[e] = (e < cnt) ? srow[b * C + o0 + e] : ~0u;
        }
        __syncthreads();
        for (unsigned int k = 2; k <= n2; k <<= 1)
            for (unsigned int j = k >> 1; j > 0; j >>= 1) {
                for (unsigned int p = t; p < n2 / 2; p += 256) {
                    const unsigned int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    const unsigned long long ka = sk[i], kb = sk[i + j];
                    const unsigned int ia = si[i], ib = si[i + j];
                    const bool gt = (ka > kb) || (ka == kb && ia > ib);
                    if (gt == ((i & k) == 0)) { sk[i] = kb; sk[i + j] = ka; si[i] = ib; si[i + j] = ia; }
                }
                __syncthreads();
            }
        for (unsigned int e = t; e < keep; e += 256) {
            idx[b * K + o0 + e] = (uint64_t)si[e];
            if (dist) dist[b * K + o0 + e] = tg_dist(sk[e]);
        }
    }
}

// the exact path of one target: its distances from the scores (the same chain)
__global__ __launch_bounds__(256) void k_tg_dist_one(const double* __restrict__ S, size_t n, size_t sld, int A,
                                                     const double* __restrict__ model, const double* __restrict__ o,
                                                     double* __restrict__ dist) {
    const int nc = tg_ncomp(model, A);
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double d2 = 0.0;
        for (int k = 0; k < nc; k++) { const double d = S[i + sld * (size_t)k] - o[k]; d2 = fma(d, d, d2); }
        dist[i] = sqrt(d2);
    }
}

// the first K of the K + 1 selected rows that are not the excluded one
__global__ __launch_bounds__(256) void k_tg_drop(const uint64_t* __restrict__ sidx, const double* __restrict__ sdist, size_t K,
                                                 const unsigned long long* __restrict__ excl, size_t b, uint64_t* __restrict__ idx,
                                                 double* __restrict__ dist) {
    __shared__ size_t s_pos;
    if (threadIdx.x == 0) {
        s_pos = K;
        for (size_t e = 0; e < K; e++)
            if (sidx[e] == (uint64_t)excl[b]) { s_pos = e; break; }
    }
    __syncthreads();
    const size_t pos = s_pos;
    for (size_t e = threadIdx.x; e < K; e += 256) {
        const size_t from = e < pos ? e : e + 1;
        idx[b * K + e] = sidx[from];
        if (dist) dist[b * K + e] = sdist[from];
    }
}

// post_mean[b P + j] = mean of Y[idx[b K + e], j] over e < K (fp64)
// RW (row importance weights, abc_ctx_set_row_weights): sum om_e Y_e / sum om_e.  Thread t takes the entries e = t, t + 256, ...
// ascending (the numerator one fma chain, the weights' sum a second chain), then both go through the same halving tree: the order is
// fixed by K alone.  0 / 0 = NaN when every om_e is 0.
template <bool RW>
__global__ __launch_bounds__(256) void k_tg_post_mean(const double* __restrict__ Y, size_t ldy, int P, const uint64_t* __restrict__ idx,
                                                      size_t K, double* __restrict__ pm, const double* __restrict__ om) {
    __shared__ double red[RW ? 512 : 256];                          // RW: the weights' sums behind the numerators
    [[maybe_unused]] double* redw = red + 256;                                    // (RW instances only)
    const size_t b = blockIdx.x;
    const int t = threadIdx.x;
    for (int j = 0; j < P; j++) {
        double s = 0.0, sw = 0.0;
        if constexpr (RW) {
            for (size_t e = t; e < K; e += 256) {
                const size_t i = (size_t)idx[b * K + e];
                const double w = om[i];
                s = fma(w, Y[i + ldy * (size_t)j], s);
                sw += w;
            }
            redw[t] = sw;
        } else {
            for (size_t e = t; e < K; e += 256) s += Y[idx[b * K + e] + ldy * (size_t)j];
        }
        red[t] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w) {
                red[t] += red[t + w];
                if constexpr (RW) redw[t] += redw[t + w];
            }
            __syncthreads();
        }
        if (t == 0) pm[b * P + j] = RW ? red[0] / redw[0] : red[0] / (double)K;
        __syncthreads();
    }
}

// the row weights' check: out[0] entries that are negative or not finite, out[1] positive entries, out[2] sum, out[3] sum of
// squares (over the valid entries).  One work-group: thread t takes the entries t, t + 1024, ... ascending, then a halving tree, so
// the sums depend on N only.
__global__ __launch_bounds__(1024) void k_rw_check(const double* __restrict__ w, size_t N, double* __restrict__ out) {
    __shared__ double r0[1024], r1[1024], r2[1024], r3[1024];
    const int t = threadIdx.x;
    double bad = 0.0, pos = 0.0, s1 = 0.0, s2 = 0.0;
    for (size_t i = t; i < N; i += 1024) {
        const double v = w[i];
        if (!(v >= 0.0) || !isfinite(v)) {
            bad += 1.0;
            continue;
        }
        if (v > 0.0) pos += 1.0;
        s1 += v;
        s2 = fma(v, v, s2);
    }
    r0[t] = bad; r1[t] = pos; r2[t] = s1; r3[t] = s2;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (t < h) { r0[t] += r0[t + h]; r1[t] += r1[t + h]; r2[t] += r2[t + h]; r3[t] += r3[t + h]; }
        __syncthreads();
    }
    if (t == 0) { out[0] = r0[0]; out[1] = r1[0]; out[2] = r2[0]; out[3] = r3[0]; }
}

// rows per thread of the candidate pass: as many as 32 score registers hold, at most four
constexpr int tg_rpt(int kc) { return (kc == 0 || kc >= 32) ? 1 : (32 / kc > 4 ? 4 : 32 / kc); }

// the padded component count the candidate pass holds in registers (0: more than 32, read as needed)
int tg_kc(size_t A) {
    const int kc = abc_project_kc(A);
    return kc > 32 ? 0 : kc;
}

struct TgPlan {
    int ns, q;          // sampled rows, rank of the threshold among them
    size_t C;           // candidate capacity per target
};

TgPlan tg_plan(size_t N, size_t K, bool any_excl) {
    TgPlan p;
    p.ns = (N < (size_t)TG_S) ? (int)N : TG_S;
    const size_t Kx = K + (any_excl ? 1 : 0);
    if ((size_t)p.ns == N) {                            // every row sampled: the exact K-th key (excluded row left out)
        p.q = (int)(K - 1);
        p.C = N;
        return p;
    }
    const double f = (double)Kx / (double)N;
    const double qd = f * TG_S + 4.0 * sqrt(TG_S * f * (1.0 - f)) + 8.0;
    p.q = (qd >= (double)(TG_S - 1)) ? TG_S - 1 : (int)qd;
    // the share of rows at or below the sample's q-th key is Beta(q + 1, S - q) distributed: mean + 8 standard deviations
    const double frac = (p.q + 1.0) / TG_S + 8.0 * sqrt(p.q + 1.0) / TG_S;
    const double cap = frac * (double)N + 256.0;
    p.C = (cap >= (double)N) ? N : (size_t)cap;
    if (p.C < K) p.C = K;
    return p;
}

const size_t TG_CHUNK_BYTES = (size_t)512 << 20;      // candidate buffers of one chunk of targets

size_t tg_chunk(const TgPlan& p, size_t B) {
    const size_t per = p.C * 24 + (TG_NB + 1) * 4;
    size_t bc = TG_CHUNK_BYTES / per;
    if (bc < 1) bc = 1;
    return bc < B ? bc : B;
}

}  // namespace

// workspace of launch_rank_targets beyond what the fallback's selection needs (abc_ws_need)
size_t abc_targets_need(size_t N, size_t A, size_t B, size_t K, bool any_excl) {
    const TgPlan p = tg_plan(N, K, any_excl);
    const int kc = tg_kc(A);
    const size_t KCO = kc ? (size_t)kc : A;
    const size_t bc = tg_chunk(p, B);
    size_t b = 0;
    b += B * KCO * 8 + B * sizeof(TgInfo) + B * 4 + B * TG_CSTRIDE * 4 + 64;          // target scores, infos, fail flags, counters, bad flag
    b += N * A * 8 + N * 8;                                              // scores of every row, distances of the fused kernel
    b += (size_t)TG_S * KCO * 8;                                         // sampled scores
    b += bc * (p.C * 24 + (TG_NB + 1) * 4);                              // candidate segments, scattered copy, bin offsets
    b += 2 * (K + 1) * 8;                                                // fallback: K + 1 selected rows
    return b + 16 * 256;
}

int launch_rank_targets(abc_ctx* ctx, const double* X, size_t ldx, const double* Y, size_t ldy, size_t N, size_t M, size_t P,
                        const double* model, size_t A, const double* targets, size_t ldt, size_t B, const uint64_t* exclude,
                        bool any_excl, size_t K, uint64_t* idx, double* dist, double* post_mean, abc_tg_scores* keep, const double* om) {
    const ModelLayout ML = model_layout(M, P, A);
    const int kc = tg_kc(A);
    const int KCO = kc ? kc : (int)A;
    const TgPlan pl = tg_plan(N, K, any_excl);
    const unsigned long long* excl = any_excl ? (const unsigned long long*)exclude : nullptr;

    double* O = (double*)abc_ws_alloc(ctx, B * KCO * 8);
    TgInfo* info = (TgInfo*)abc_ws_alloc(ctx, B * sizeof(TgInfo));
    int* fail = (int*)abc_ws_alloc(ctx, B * 4);
    unsigned int* cnt = (unsigned int*)abc_ws_alloc(ctx, B * TG_CSTRIDE * 4);
    int* bad = (int*)abc_ws_alloc(ctx, 64);
    double* S = (double*)abc_ws_alloc(ctx, N * A * 8);
    double* dtmp = (double*)abc_ws_alloc(ctx, N * 8);
    double* Ss = (double*)abc_ws_alloc(ctx, (size_t)TG_S * KCO * 8);
    if (!O || !info || !fail || !cnt || !bad || !S || !dtmp || !Ss) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets: workspace exhausted");
    if (keep) { keep->S = S; keep->sld = N; keep->O = O; keep->KCO = KCO; }     // (the arena keeps them past the return)

    // target scores; non-finite targets are refused before anything else runs
    ABC_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_tg_scores, dim3((unsigned)((B * KCO + 255) / 256)), dim3(256), 0, ctx->stream, targets, ldt, B, (int)M, (int)A,
                       KCO, model, ML.off_mean, ML.off_sd, ML.off_R, O, bad);
    ABC_HIP(ctx, hipGetLastError());
    int bad_h = 0;
    ABC_HIP(ctx, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad_h) ABC_FAIL(ctx, ABC_ERR_INVALID, "rank_targets: a target holds a non-finite metric");

    // scores of every row
    {
        StageTimer tm(ctx, ST_PROJECT);
        if (launch_project_distance_scores(ctx, X, N, ldx, M, P, A, model, dtmp, S, N, 0, nullptr) != 0) {
            size_t blocks = (N + 255) / 256;
            if (blocks > 4096) blocks = 4096;
            hipLaunchKernelGGL(k_tg_row_scores, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, X, N, ldx, (int)M, (int)A, model,
                               ML.off_mean, ML.off_sd, ML.off_R, S, N);
        }
        ABC_HIP(ctx, hipGetLastError());
    }

    StageTimer tm(ctx, ST_SELECT);
    ABC_HIP(ctx, hipMemsetAsync(fail, 0, B * 4, ctx->stream));
    ABC_HIP(ctx, hipMemsetAsync(cnt, 0, B * TG_CSTRIDE * 4, ctx->stream));
    hipLaunchKernelGGL(k_tg_sample, dim3((unsigned)((pl.ns * KCO + 255) / 256)), dim3(256), 0, ctx->stream, S, N, N, pl.ns, (int)A, KCO,
                       model, Ss);
    hipLaunchKernelGGL(k_tg_threshold, dim3((unsigned)B), dim3(1024), 0, ctx->stream, Ss, N, pl.ns, pl.q, KCO, O, excl, info);
    ABC_HIP(ctx, hipGetLastError());

    const size_t bc = tg_chunk(pl, B), C = pl.C;
    const size_t mark = ctx->ws_off;
    unsigned long long* ckey = (unsigned long long*)abc_ws_alloc(ctx, bc * C * 8);
    unsigned long long* skey = (unsigned long long*)abc_ws_alloc(ctx, bc * C * 8);
    unsigned int* crow = (unsigned int*)abc_ws_alloc(ctx, bc * C * 4);
    unsigned int* srow = (unsigned int*)abc_ws_alloc(ctx, bc * C * 4);
    unsigned int* offs = (unsigned int*)abc_ws_alloc(ctx, bc * (TG_NB + 1) * 4);
    if (!ckey || !skey || !crow || !srow || !offs) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets: workspace exhausted");
    const size_t rb = (N + 256 * tg_rpt(kc) - 1) / (256 * tg_rpt(kc));
    for (size_t c0 = 0; c0 < B; c0 += bc) {
        const size_t nb = (B - c0 < bc) ? B - c0 : bc;
        // target groups: enough work-groups to fill the chip when the rows alone do not
        size_t groups = (rb >= 2048) ? 1 : (2048 + rb - 1) / rb;
        if (groups > nb) groups = nb;
        const size_t tgs = (nb + groups - 1) / groups;
        groups = (nb + tgs - 1) / tgs;
        const unsigned long long* ex = excl ? excl + c0 : nullptr;
#define TG_CAND(KCV)                                                                                                        \
    hipLaunchKernelGGL((k_tg_cand<KCV, tg_rpt(KCV)>), dim3((unsigned)((N + 256 * tg_rpt(KCV) - 1) / (256 * tg_rpt(KCV))),  \
                       (unsigned)groups), dim3(256), 0, ctx->stream, S, N, N, (int)A, KCO, model, O + c0 * KCO, nb, tgs, ex,     \
                       info + c0, C, cnt + c0 * TG_CSTRIDE, ckey, crow)
        switch (kc) {
            case 1: TG_CAND(1); break;
            case 2: TG_CAND(2); break;
            case 4: TG_CAND(4); break;
            case 8: TG_CAND(8); break;
            case 16: TG_CAND(16); break;
            case 32: TG_CAND(32); break;
            default: TG_CAND(0); break;
        }
#undef TG_CAND
        ABC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_tg_bins, dim3((unsigned)nb), dim3(1024), 0, ctx->stream, (const unsigned int*)(cnt + c0 * TG_CSTRIDE), C,
                           (unsigned long long)K, info + c0, fail + c0, (const unsigned long long*)ckey, (const unsigned int*)crow, offs,
                           skey, srow);
        hipLaunchKernelGGL(k_tg_sort, dim3(64, (unsigned)nb), dim3(256), 0, ctx->stream, (const TgInfo*)(info + c0),
                           (const int*)(fail + c0), (const unsigned int*)offs, (const unsigned long long*)skey, (const unsigned int*)srow, C,
                           (unsigned long long)K, idx + c0 * K, dist ? dist + c0 * K : nullptr);
        ABC_HIP(ctx, hipGetLastError());
    }
    ctx->ws_off = mark;

    // targets the batched selection gave up on: the exact single-target path
    std::vector<int> fail_h(B);
    ABC_HIP(ctx, hipMemcpyAsync(fail_h.data(), fail, B * 4, hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> ex_h;
    for (size_t b = 0; b < B; b++) {
        if (!fail_h[b]) continue;
        ctx->targets_fallbacks++;
        if (excl && ex_h.empty()) {
            ex_h.resize(B);
            ABC_HIP(ctx, hipMemcpyAsync(ex_h.data(), excl, B * 8, hipMemcpyDeviceToHost, ctx->stream));
            ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        const bool drop = excl && ex_h[b] != ~0ull;
        size_t blocks = (N + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_tg_dist_one, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, S, N, N, (int)A, model, O + b * KCO, dtmp);
        ABC_HIP(ctx, hipGetLastError());
        const size_t fm = ctx->ws_off;
        if (!drop) {
            ABC_TRY(launch_select_smallest(ctx, dtmp, N, K, 0, idx + b * K, dist ? dist + b * K : nullptr, false));
        } else {
            uint64_t* si = (uint64_t*)abc_ws_alloc(ctx, (K + 1) * 8);
            double* sd = (double*)abc_ws_alloc(ctx, (K + 1) * 8);
            if (!si || !sd) ABC_FAIL(ctx, ABC_ERR_NOMEM, "rank_targets: workspace exhausted");
            ABC_TRY(launch_select_smallest(ctx, dtmp, N, K + 1, 0, si, sd, false));
            hipLaunchKernelGGL(k_tg_drop, dim3(1), dim3(256), 0, ctx->stream, (const uint64_t*)si, (const double*)sd, K, excl, b, idx, dist);
            ABC_HIP(ctx, hipGetLastError());
        }
        ctx->ws_off = fm;
    }
    if (post_mean && P) {
        hipLaunchKernelGGL(om ? k_tg_post_mean<true> : k_tg_post_mean<false>, dim3((unsigned)B), dim3(256), 0, ctx->stream, Y, ldy, (int)P,
                           (const uint64_t*)idx, K, post_mean, om);
        ABC_HIP(ctx, hipGetLastError());
    }
    return ABC_OK;
}

int launch_row_weights_check(abc_ctx* ctx, const double* w_dev, size_t N, double* out4_dev) {
    hipLaunchKernelGGL(k_rw_check, dim3(1), dim3(1024), 0, ctx->stream, w_dev, N, out4_dev);
    ABC_HIP(ctx, hipGetLastError());
    return ABC_OK;
}
