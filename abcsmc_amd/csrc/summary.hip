// Weighted posterior quantiles and CDF of segments (abc_rank_targets_summary_dev, abc_weighted_summary_dev; the definition is in
// the header).  A segment is one (target b, parameter j); its K values and weights are made by segment_dev.h.
//
// The key of a value is its order-preserving 64-bit image (IEEE totalOrder); an entry of weight 0 gets the key ~0 and sorts
// behind every finite value.  A segment's entries are sorted by (key, e), then one pass in tiles of SM_TILE sorted entries makes
// the running weight sums and the knots' numerators H_r = fma(-0.5, om_r, W_r), and the CDF's sums L and E; every level q is
// then one binary search over the knots.
//   LDS path    (K <= SM_LDS_MAX)  k_sm_lds: one work-group per segment; keys and e sorted by a bitonic sort in LDS, the knots
//                                  written over the sorted e
//   global path (larger K)         k_sm_chunk sorts chunks of SM_LDS_MAX entries in LDS the same way and writes them out,
//                                  k_sm_merge merges runs pairwise (an entry's place is its rank in its own run plus its rank in
//                                  the partner run: (key, e) is unique within a segment), k_sm_eval_global evaluates as above
// The sums run in an order fixed by the tile (SM_TILE entries, SM_PER consecutive ones per thread, a fixed scan and tree over the
// threads, tiles in order) and nothing else, so both paths give the same bits for any weights, a target's bits do not depend on the
// batch, and no floating-point atomics are involved.
//
// Tolerance paths (abc_rank_targets_path_summary_dev).  Under rejection the values do not depend on the tolerance and the tie-break
// is the entry number, so the (key, e) list sorted at K_max, filtered by e < K_t, is the sorted segment at K_t: ONE sort per
// (target, parameter), then k_smp_lds / k_smp_eval_global walk the tolerances from the largest down, evaluate the n = K_t dense
// entries and compact them (stable, by an integer count scan) to those with e < K_{t-1}.  With unit weights sm_eval's knot numerator
// of rank r is exactly r + 0.5 and W = n, so no H array is kept; the expressions are sm_eval's.  Under loclinear the values change
// with the tolerance (its own beta): segment (b, t, j) goes through the kernels above with K = K_t, the row stride K_max and the
// coefficient and output slot b T + t (SmArgs ld, T, t).
//
// Highest-density intervals (abc_rank_targets_hpd_dev, abc_weighted_hpd_dev): the same sort and the same knots, then per mass the
// shortest of the 2 n candidate intervals that end on a knot (k_hp_lds; k_hp_knots_global, k_hp_search_global, k_hp_final_global).
#include <math.h>

#include "abc_internal.h"
#include "segment_dev.h"

namespace {

constexpr int SM_BS = 512;                                  // threads of every summary work-group
constexpr int SM_PER = 16;                                  // consecutive sorted entries per thread and tile
constexpr int SM_TILE = SM_BS * SM_PER;                     // 8192
constexpr int SM_LDS_MAX = 8192;                            // largest K of the LDS path; also the chunk of the global path
constexpr int SM_MAXQ = 64;
constexpr size_t SM_WS_BYTES = (size_t)256 << 20;           // sort buffers of one batch of targets (global path)
constexpr unsigned SM_MAX_GRID_Y = 65535;
constexpr unsigned long long SM_PAD_KEY = ~0ull;
constexpr unsigned SM_PAD_ID = 0xFFFFFFFFu;

struct SmProbs {
    double q[SM_MAXQ];
    int nq;
};

__device__ __forceinline__ unsigned long long sm_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double sm_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}
__device__ __forceinline__ bool sm_less(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// entries e0 .. e0 + len - 1 of the segment as (key, e) pairs in key[0..n2) / id[0..n2) (n2 a power of two >= len, padding behind),
// sorted ascending by a bitonic sort; the count of positive weights and a non-finite flag added to *cnt / *bad
template <bool TF = true, bool HC = false>
__device__ void sm_build_sort(const SmArgs& a, const SmSeg& s, size_t e0, int len, int n2, unsigned long long* key, unsigned* id,
                              unsigned* cnt, int* bad) {
    const int t = threadIdx.x;
    unsigned c = 0;
    int nf = 0;
    for (int r = t; r < n2; r += SM_BS) {
        unsigned long long k = SM_PAD_KEY;
        unsigned i = SM_PAD_ID;
        if (r < len) {
            const size_t e = e0 + (size_t)r;
            const double v = sm_value<TF, HC>(a, s, e);
            if (!isfinite(v)) nf = 1;
            i = (unsigned)e;
            if (sm_weight(a, s, e) > 0.0) {
                k = sm_key(v);
                c++;
            }
        }
        key[r] = k;
        id[r] = i;
    }
    if (c) atomicAdd(cnt, c);
    if (nf) atomicOr(bad, 1);
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int p = t; p < n2 / 2; p += SM_BS) {
                const int i = (p / jj) * 2 * jj + (p % jj), l = i + jj;
                const bool asc = (i & k) == 0;
                const unsigned long long ki = key[i], kl = key[l];
                const unsigned ii = id[i], il = id[l];
                if (sm_less(kl, il, ki, ii) == asc) {
                    key[i] = kl; key[l] = ki;
                    id[i] = il; id[l] = ii;
                }
            }
            __syncthreads();
        }
}

// the evaluation of one segment from its n sorted entries with positive weight (key[r], id[r]); H (n entries) receives the knots'
// numerators and may overlay id from byte 0 of id (the LDS path; only one tile there).  red: 3 x SM_BS doubles of LDS.
__device__ void sm_eval(const SmArgs& a, const SmSeg& s, const SmProbs& pr, const unsigned long long* key, const unsigned* id,
                        double* H, size_t n, bool bad, double* red) {
    const int t = threadIdx.x;
    double* scan = red;
    double* rl = red + SM_BS;
    double* re = red + 2 * SM_BS;
    const double tau = a.cdf ? a.truth[s.b * a.P + s.j] : 0.0;
    double carry = 0.0, L = 0.0, E = 0.0;
    for (size_t base = 0; base < n; base += SM_TILE) {
        const size_t r0 = base + (size_t)t * SM_PER;
        double om[SM_PER], inc[SM_PER];
        double acc = 0.0, lt = 0.0, et = 0.0;
#pragma unroll
        for (int q = 0; q < SM_PER; q++) {
            const size_t r = r0 + q;
            om[q] = 0.0;
            if (r < n) {
                om[q] = sm_weight(a, s, (size_t)id[r]);
                const double u = sm_unkey(key[r]);
                if (u < tau) lt += om[q];
                else if (u == tau) et += om[q];
            }
            acc += om[q];
            inc[q] = acc;
        }
        scan[t] = acc;
        rl[t] = lt;
        re[t] = et;
        __syncthreads();                                       // (also: every id of the tile is read before H is written)
        for (int off = 1; off < SM_BS; off <<= 1) {
            const double v = (t >= off) ? scan[t - off] : 0.0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        for (int st = SM_BS / 2; st > 0; st >>= 1) {
            if (t < st) {
                rl[t] += rl[t + st];
                re[t] += re[t + st];
            }
            __syncthreads();
        }
        const double off = carry + ((t > 0) ? scan[t - 1] : 0.0);
#pragma unroll
        for (int q = 0; q < SM_PER; q++) {
            const size_t r = r0 + q;
            if (r < n) H[r] = fma(-0.5, om[q], off + inc[q]);
        }
        carry += scan[SM_BS - 1];
        L += rl[0];
        E += re[0];
        __syncthreads();                                       // scan / rl / re read before the next tile writes them
    }
    __syncthreads();                                           // H complete
    const double W = carry;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int qi = t; qi < pr.nq; qi += SM_BS) {
        const double q = pr.q[qi];
        double res;
        if (bad || n == 0) {
            res = nan;
        } else if (q <= H[0] / W) {
            res = sm_unkey(key[0]);
        } else if (q >= H[n - 1] / W) {
            res = sm_unkey(key[n - 1]);
        } else {                                               // p_lo <= q < p_hi
            size_t lo = 0, hi = n - 1;
            while (hi - lo > 1) {
                const size_t mid = lo + (hi - lo) / 2;
                if (H[mid] / W <= q) lo = mid; else hi = mid;
            }
            const double plo = H[lo] / W, phi = H[hi] / W;
            const double tt = (q - plo) / (phi - plo);
            const double ulo = sm_unkey(key[lo]), uhi = sm_unkey(key[hi]);
            res = fma(tt, uhi - ulo, ulo);
        }
        if (a.quant) a.quant[(s.slot * (size_t)pr.nq + qi) * a.P + s.j] = res;
    }
    if (a.cdf && t == 0) a.cdf[s.slot * a.P + s.j] = (bad || n == 0 || isnan(tau)) ? nan : fma(0.5, E, L) / W;
}

// LDS path: grid (P, targets b0 + blockIdx.y); dynamic LDS 16 n2 bytes: keys (8 n2), then e (4 n2) overlaid by H (8 n2).  HC (here
// and in k_sm_chunk): the values under the variance correction, an instance the launcher takes only when a.hcoef is set
template <bool HC>
__global__ __launch_bounds__(SM_BS) void k_sm_lds(SmArgs a, SmProbs pr, int n2, size_t b0) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long smk[];
    __shared__ double red[3 * SM_BS];
    __shared__ unsigned s_cnt;
    __shared__ int s_bad;
    unsigned long long* key = smk;
    unsigned* id = (unsigned*)(smk + n2);
    double* H = (double*)(smk + n2);
    if (threadIdx.x == 0) { s_cnt = 0; s_bad = 0; }
    __syncthreads();
    const SmSeg s = sm_seg<HC>(a, b0 + blockIdx.y, (int)blockIdx.x);
    sm_build_sort<true, HC>(a, s, 0, (int)a.K, n2, key, id, &s_cnt, &s_bad);
    sm_eval(a, s, pr, key, id, H, (size_t)s_cnt, s_bad != 0, red);
}

// global path, 1: grid (chunks x P, batch targets); chunk c of segment (bl, j) sorted in LDS and written to key / id at
// seg K + c SM_LDS_MAX, seg = bl P + j; positive weights counted into cnt[seg], non-finite values flagged in bad[seg]
template <bool HC>
__global__ __launch_bounds__(SM_BS) void k_sm_chunk(SmArgs a, size_t b0, unsigned long long* __restrict__ gkey, unsigned* __restrict__ gid,
                                                    unsigned* __restrict__ cnt, int* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long key[];   // SM_LDS_MAX keys, then SM_LDS_MAX e
    unsigned* id = (unsigned*)(key + SM_LDS_MAX);
    const int j = (int)(blockIdx.x % (unsigned)a.P);
    const size_t c = blockIdx.x / (unsigned)a.P, bl = blockIdx.y;
    const size_t e0 = c * SM_LDS_MAX;
    const int len = (a.K - e0 < (size_t)SM_LDS_MAX) ? (int)(a.K - e0) : SM_LDS_MAX;
    int n2 = 1;
    while (n2 < len) n2 <<= 1;
    const size_t seg = bl * a.P + j;
    const SmSeg s = sm_seg<HC>(a, b0 + bl, j);
    sm_build_sort<true, HC>(a, s, e0, len, n2, key, id, cnt + seg, bad + seg);
    unsigned long long* ok = gkey + seg * a.K + e0;
    unsigned* oi = gid + seg * a.K + e0;
    for (int r = threadIdx.x; r < len; r += SM_BS) {
        ok[r] = key[r];
        oi[r] = id[r];
    }
}

// global path, 2: runs of w entries of every segment merged pairwise (in -> out), one thread per entry
__global__ __launch_bounds__(256) void k_sm_merge(const unsigned long long* __restrict__ ik, const unsigned* __restrict__ ii, size_t K,
                                                  size_t total, size_t w, unsigned long long* __restrict__ okey,
                                                  unsigned* __restrict__ oid) {
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
        const size_t seg = g / K, i = g % K, run = i / w, start = run * w, ps = (run ^ 1) * w;
        const unsigned long long k = ik[g];
        const unsigned d = ii[g];
        size_t pos = i;
        if (ps < K) {
            const size_t pe = (ps + w < K) ? ps + w : K;
            const unsigned long long* pk = ik + seg * K;
            const unsigned* pi = ii + seg * K;
            size_t lo = ps, hi = pe;                            // entries of the partner run below (k, d)
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (sm_less(pk[mid], pi[mid], k, d)) lo = mid + 1; else hi = mid;
            }
            pos = (start < ps ? start : ps) + (i - start) + (lo - ps);
        }
        okey[seg * K + pos] = k;
        oid[seg * K + pos] = d;
    }
}

// global path, 3: grid (P, batch targets); H: the other key buffer
__global__ __launch_bounds__(SM_BS) void k_sm_eval_global(SmArgs a, SmProbs pr, size_t b0, const unsigned long long* __restrict__ gkey,
                                                          const unsigned* __restrict__ gid, double* __restrict__ gH,
                                                          const unsigned* __restrict__ cnt, const int* __restrict__ bad) {
    __shared__ double red[3 * SM_BS];
    const int j = (int)blockIdx.x;
    const size_t bl = blockIdx.y, seg = bl * a.P + j;
    const SmSeg s = sm_seg(a, b0 + bl, j);
    sm_eval(a, s, pr, gkey + seg * a.K, gid + seg * a.K, gH + seg * a.K, (size_t)cnt[seg], bad[seg] != 0, red);
}

// ---- highest-density intervals (abc_rank_targets_hpd_dev, abc_weighted_hpd_dev; the definition is in the header) ----
// The sort is the summary's and so are the knots: hp_knots repeats sm_eval's tile pass expression for expression (without the CDF's
// sums, which do not enter H), then p_r = H_r / W is stored once over H, the bits sm_eval compares.  Every mass is one sweep of the
// work-group over the 2 n candidates (one binary search over p each) and one reduction of the pair (width, c), whose order is
// total: the winner does not depend on the reduction's shape (on the global path the candidates are split over work-groups).
constexpr int HP_MAXM = 16;
constexpr unsigned long long HP_NONE = ~0ull;               // the candidate number of "no valid candidate"

struct HpMass {
    double m[HP_MAXM];
    int nm;
};
struct HpOut {
    double *lo, *hi, *plo, *phi;                            // B x nm x P each, NULL: not asked for
};

// sm_eval's tile pass: H[r] = fma(-0.5, om_r, W_r) for the n sorted entries, the same per-thread order, scan and carry; returns W.
// H may overlay id from byte 0 of id (the LDS path; only one tile there).  scan: SM_BS doubles of LDS.
__device__ double hp_knots(const SmArgs& a, const SmSeg& s, const unsigned* id, double* H, size_t n, double* scan) {
    const int t = threadIdx.x;
    double carry = 0.0;
    for (size_t base = 0; base < n; base += SM_TILE) {
        const size_t r0 = base + (size_t)t * SM_PER;
        double om[SM_PER], inc[SM_PER];
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < SM_PER; q++) {
            const size_t r = r0 + q;
            om[q] = 0.0;
            if (r < n) om[q] = sm_weight(a, s, (size_t)id[r]);
            acc += om[q];
            inc[q] = acc;
        }
        scan[t] = acc;
        __syncthreads();                                       // (also: every id of the tile is read before H is written)
        for (int off = 1; off < SM_BS; off <<= 1) {
            const double v = (t >= off) ? scan[t - off] : 0.0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const double off = carry + ((t > 0) ? scan[t - 1] : 0.0);
#pragma unroll
        for (int q = 0; q < SM_PER; q++) {
            const size_t r = r0 + q;
            if (r < n) H[r] = fma(-0.5, om[q], off + inc[q]);
        }
        carry += scan[SM_BS - 1];
        __syncthreads();                                       // scan read before the next tile writes it
    }
    __syncthreads();                                           // H complete
    return carry;
}

// the summary's quantile function over the stored knots p (sm_eval's expressions with p[r] for H[r] / W), n >= 1
__device__ __forceinline__ double hp_quantile(const double* p, const unsigned long long* key, size_t n, double q) {
    if (q <= p[0]) return sm_unkey(key[0]);
    if (q >= p[n - 1]) return sm_unkey(key[n - 1]);
    size_t lo = 0, hi = n - 1;                                 // p_lo <= q < p_hi
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (p[mid] <= q) lo = mid; else hi = mid;
    }
    const double plo = p[lo], phi = p[hi];
    const double tt = (q - plo) / (phi - plo);
    const double ulo = sm_unkey(key[lo]), uhi = sm_unkey(key[hi]);
    return fma(tt, uhi - ulo, ulo);
}

// candidate c = 2 r + kind of mass m; false: not valid (the outputs are then not set)
__device__ __forceinline__ bool hp_cand(const double* p, const unsigned long long* key, size_t n, double m, unsigned long long c,
                                        double p0, double pl, double* lo, double* hi, double* plo, double* phi) {
    const size_t r = (size_t)(c >> 1);
    const double pr = p[r], ur = sm_unkey(key[r]);
    if ((c & 1) == 0) {                                        // lower end on knot r
        const double q = pr + m;
        if (!(q <= pl)) return false;
        *plo = pr; *phi = q;
        *lo = ur; *hi = hp_quantile(p, key, n, q);
    } else {                                                   // upper end on knot r
        const double q = pr - m;
        if (!(q >= p0)) return false;
        *plo = q; *phi = pr;
        *lo = hp_quantile(p, key, n, q); *hi = ur;
    }
    return true;
}

// the best (width, c) over the candidates c0 <= c < c1 of mass m, the work-group's threads striding over them; the result is
// thread 0's alone.  rw / rc: SM_BS / 64 entries of LDS each, free again after the return
__device__ void hp_sweep(const double* p, const unsigned long long* key, size_t n, double m, unsigned long long c0, unsigned long long c1,
                         double p0, double pl, double* rw, unsigned long long* rc, double* bw_out, unsigned long long* bc_out) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double bw = __longlong_as_double(0x7ff0000000000000ll);
    unsigned long long bc = HP_NONE;
    double lo, hi, plo, phi;
    for (unsigned long long c = c0 + (unsigned long long)t; c < c1; c += SM_BS)
        if (hp_cand(p, key, n, m, c, p0, pl, &lo, &hi, &plo, &phi)) {
            const double w = hi - lo;
            if (w < bw || (w == bw && c < bc)) { bw = w; bc = c; }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double w2 = __shfl_down(bw, off, 64);
        const unsigned long long c2 = __shfl_down(bc, off, 64);
        if (w2 < bw || (w2 == bw && c2 < bc)) { bw = w2; bc = c2; }
    }
    if (lane == 0) { rw[wave] = bw; rc[wave] = bc; }
    __syncthreads();
    if (t == 0)
        for (int v = 1; v < SM_BS / 64; v++)
            if (rw[v] < bw || (rw[v] == bw && rc[v] < bc)) { bw = rw[v]; bc = rc[v]; }
    __syncthreads();                                           // rw / rc read before the next sweep writes them
    *bw_out = bw;
    *bc_out = bc;
}

// one thread: the four outputs of (slot, mass mi, parameter j) from the winner bc (HP_NONE: none was valid); none: all NaN
__device__ void hp_store(const HpOut& o, size_t at, const double* p, const unsigned long long* key, size_t n, double m,
                         unsigned long long bc, bool none, double p0, double pl) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double lo = nan, hi = nan, plo = nan, phi = nan;
    if (!none) {
        if (bc == HP_NONE) {                                   // n = 1, or m at least the knots' span
            lo = sm_unkey(key[0]); hi = sm_unkey(key[n - 1]);
            plo = p0; phi = pl;
        } else {
            hp_cand(p, key, n, m, bc, p0, pl, &lo, &hi, &plo, &phi);
        }
    }
    if (o.lo) o.lo[at] = lo;
    if (o.hi) o.hi[at] = hi;
    if (o.plo) o.plo[at] = plo;
    if (o.phi) o.phi[at] = phi;
}

// the knots of one segment over H: p_r = H_r / W.  scan: SM_BS doubles of LDS
__device__ void hp_make_knots(const SmArgs& a, const SmSeg& s, const unsigned* id, double* H, size_t n, double* scan) {
    const double W = hp_knots(a, s, id, H, n, scan);
    for (size_t r = threadIdx.x; r < n; r += SM_BS) H[r] = H[r] / W;
    __syncthreads();
}

// LDS path: k_sm_lds's grid and dynamic LDS
template <bool HC>
__global__ __launch_bounds__(SM_BS) void k_hp_lds(SmArgs a, HpMass hm, HpOut o, int n2, size_t b0) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long smk[];
    __shared__ double red[3 * SM_BS];
    __shared__ unsigned s_cnt;
    __shared__ int s_bad;
    unsigned long long* key = smk;
    unsigned* id = (unsigned*)(smk + n2);
    double* H = (double*)(smk + n2);
    if (threadIdx.x == 0) { s_cnt = 0; s_bad = 0; }
    __syncthreads();
    const SmSeg s = sm_seg<HC>(a, b0 + blockIdx.y, (int)blockIdx.x);
    sm_build_sort<true, HC>(a, s, 0, (int)a.K, n2, key, id, &s_cnt, &s_bad);
    const size_t n = (size_t)s_cnt;
    const bool none = s_bad != 0 || n == 0;
    hp_make_knots(a, s, id, H, n, red);
    const double p0 = none ? 0.0 : H[0], pl = none ? 0.0 : H[n - 1];
    for (int mi = 0; mi < hm.nm; mi++) {                       // (red: the scan is done, the sweeps' pairs take its place)
        double bw = 0.0;
        unsigned long long bc = HP_NONE;
        if (!none) hp_sweep(H, key, n, hm.m[mi], 0, 2ull * n, p0, pl, red, (unsigned long long*)(red + SM_BS), &bw, &bc);
        if (threadIdx.x == 0) hp_store(o, (s.slot * (size_t)hm.nm + (size_t)mi) * a.P + s.j, H, key, n, hm.m[mi], bc, none, p0, pl);
    }
}

// global path, 3: three kernels in the place of k_sm_eval_global, because a segment's 2 n candidates are n log n dependent reads of
// global memory: too long a chain for the one work-group a segment has there, and a batch holds few segments.  The order of
// (width, c) is total, so the split changes no bit.
//   k_hp_knots_global   grid (P, batch targets): the knots p into the other key buffer
//   k_hp_search_global  grid (P x HP_SPLIT, batch targets): slice sp of every mass's candidates, its best pair to
//                       pw / pc[(seg nm + mi) HP_SPLIT + sp]
//   k_hp_final_global   one thread per (segment, mass): the best of the slices' pairs, the winner evaluated again and written
constexpr int HP_SPLIT = 8;

__global__ __launch_bounds__(SM_BS) void k_hp_knots_global(SmArgs a, size_t b0, const unsigned* __restrict__ gid, double* gH,
                                                           const unsigned* __restrict__ cnt) {
    __shared__ double scan[SM_BS];
    const int j = (int)blockIdx.x;
    const size_t bl = blockIdx.y, seg = bl * a.P + j;
    const SmSeg s = sm_seg(a, b0 + bl, j);
    hp_make_knots(a, s, gid + seg * a.K, gH + seg * a.K, (size_t)cnt[seg], scan);
}

__global__ __launch_bounds__(SM_BS) void k_hp_search_global(SmArgs a, HpMass hm, const unsigned long long* __restrict__ gkey,
                                                            const double* __restrict__ gp, const unsigned* __restrict__ cnt,
                                                            const int* __restrict__ bad, double* __restrict__ pw,
                                                            unsigned long long* __restrict__ pc) {
    __shared__ double rw[SM_BS / 64];
    __shared__ unsigned long long rc[SM_BS / 64];
    const int j = (int)(blockIdx.x % (unsigned)a.P), sp = (int)(blockIdx.x / (unsigned)a.P);
    const size_t seg = (size_t)blockIdx.y * a.P + j, n = (size_t)cnt[seg];
    if (bad[seg] != 0 || n == 0) return;                       // (uniform; k_hp_final_global does not read the pairs then)
    const unsigned long long* key = gkey + seg * a.K;
    const double* p = gp + seg * a.K;
    const double p0 = p[0], pl = p[n - 1];
    const unsigned long long total = 2ull * n, per = (total + HP_SPLIT - 1) / HP_SPLIT;
    const unsigned long long c0 = (unsigned long long)sp * per, c1 = (c0 + per < total) ? c0 + per : total;
    for (int mi = 0; mi < hm.nm; mi++) {
        double bw;
        unsigned long long bc;
        hp_sweep(p, key, n, hm.m[mi], c0, c1, p0, pl, rw, rc, &bw, &bc);     // (c0 >= c1: no candidate, the pair of none)
        if (threadIdx.x == 0) {
            const size_t at = (seg * (size_t)hm.nm + (size_t)mi) * HP_SPLIT + (size_t)sp;
            pw[at] = bw;
            pc[at] = bc;
        }
    }
}

__global__ __launch_bounds__(256) void k_hp_final_global(SmArgs a, HpMass hm, HpOut o, size_t b0, size_t nseg,
                                                         const unsigned long long* __restrict__ gkey, const double* __restrict__ gp,
                                                         const unsigned* __restrict__ cnt, const int* __restrict__ bad,
                                                         const double* __restrict__ pw, const unsigned long long* __restrict__ pc) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nseg * (size_t)hm.nm) return;
    const size_t seg = g / (size_t)hm.nm, mi = g % (size_t)hm.nm, bl = seg / (size_t)a.P, j = seg % (size_t)a.P;
    const size_t n = (size_t)cnt[seg];
    const bool none = bad[seg] != 0 || n == 0;
    const unsigned long long* key = gkey + seg * a.K;
    const double* p = gp + seg * a.K;
    double bw = __longlong_as_double(0x7ff0000000000000ll);
    unsigned long long bc = HP_NONE;
    if (!none)
        for (int sp = 0; sp < HP_SPLIT; sp++) {
            const double w2 = pw[g * HP_SPLIT + sp];
            const unsigned long long c2 = pc[g * HP_SPLIT + sp];
            if (w2 < bw || (w2 == bw && c2 < bc)) { bw = w2; bc = c2; }
        }
    hp_store(o, ((b0 + bl) * (size_t)hm.nm + mi) * a.P + j, p, key, n, hm.m[mi], bc, none, none ? 0.0 : p[0], none ? 0.0 : p[n - 1]);
}

// ---- tolerance path, rejection: one sort at K_max, every tolerance from it ----
constexpr int SM_MAXT = 16;
struct SmKs {
    size_t K[SM_MAXT];
    int T;
};

// the outputs of one tolerance from its n sorted entries key[0..n), all of weight 1: sm_eval's expressions with H[r] = r + 0.5 and
// W = n (both exact); L, E: the entries below and equal to tau, nf: the non-finite ones
__device__ void smp_out(const SmArgs& a, const SmSeg& s, const SmProbs& pr, const unsigned long long* key, size_t n, bool bad, double L,
                        double E, double tau) {
    const int t = threadIdx.x;
    const double W = (double)n;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int qi = t; qi < pr.nq; qi += SM_BS) {
        const double q = pr.q[qi];
        double res;
        if (bad || n == 0) {
            res = nan;
        } else if (q <= 0.5 / W) {
            res = sm_unkey(key[0]);
        } else if (q >= ((double)(n - 1) + 0.5) / W) {
            res = sm_unkey(key[n - 1]);
        } else {                                               // p_lo <= q < p_hi
            size_t lo = 0, hi = n - 1;
            while (hi - lo > 1) {
                const size_t mid = lo + (hi - lo) / 2;
                if (((double)mid + 0.5) / W <= q) lo = mid; else hi = mid;
            }
            const double plo = ((double)lo + 0.5) / W, phi = ((double)hi + 0.5) / W;
            const double tt = (q - plo) / (phi - plo);
            const double ulo = sm_unkey(key[lo]), uhi = sm_unkey(key[hi]);
            res = fma(tt, uhi - ulo, ulo);
        }
        if (a.quant) a.quant[(s.slot * (size_t)pr.nq + qi) * a.P + s.j] = res;
    }
    if (a.cdf && t == 0) a.cdf[s.slot * a.P + s.j] = (bad || n == 0 || isnan(tau)) ? nan : fma(0.5, E, L) / W;
}

// exclusive offset of this thread's count c among the work-group's (wave scan, then the waves' sums through ws); *total: all of them.
// Two barriers: ws may be written again after the return.
__device__ __forceinline__ unsigned smp_scan(unsigned c, unsigned* ws, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    unsigned off = inc - c, tot = 0;
    for (int w = 0; w < SM_BS / 64; w++) {
        const unsigned v = ws[w];
        if (w < wave) off += v;
        tot += v;
    }
    __syncthreads();
    *total = tot;
    return off;
}

// LDS path of the tolerance path: grid (P, targets b0 + blockIdx.y); a.K = K_max; dynamic LDS 12 n2 bytes: keys (8 n2), then e (4 n2)
__global__ __launch_bounds__(SM_BS) void k_smp_lds(SmArgs a, SmProbs pr, SmKs ks, int n2, size_t b0) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long smk[];
    __shared__ unsigned s_cnt, s_ws[SM_BS / 64], s_L, s_E, s_nf;
    __shared__ int s_bad;
    unsigned long long* key = smk;
    unsigned* id = (unsigned*)(smk + n2);
    const int t = threadIdx.x;
    if (t == 0) { s_cnt = 0; s_bad = 0; }
    __syncthreads();
    SmSeg s = sm_seg(a, b0 + blockIdx.y, (int)blockIdx.x);
    sm_build_sort<false>(a, s, 0, (int)a.K, n2, key, id, &s_cnt, &s_bad);     // (rejection only: launch_path_summary)
    const double tau = a.cdf ? a.truth[s.b * a.P + s.j] : 0.0;
    for (int ti = ks.T - 1; ti >= 0; ti--) {
        const unsigned n = (unsigned)ks.K[ti], keep = ti > 0 ? (unsigned)ks.K[ti - 1] : 0u;
        if (t == 0) { s_L = 0; s_E = 0; s_nf = 0; }
        __syncthreads();
        unsigned long long kr[SM_PER];
        unsigned ir[SM_PER];
        unsigned c = 0, lt = 0, eq = 0, nf = 0;
#pragma unroll
        for (int q = 0; q < SM_PER; q++) {
            const unsigned r = (unsigned)t * SM_PER + q;
            kr[q] = SM_PAD_KEY;
            ir[q] = SM_PAD_ID;
            if (r < n) {
                kr[q] = key[r];
                ir[q] = id[r];
                const double u = sm_unkey(kr[q]);
                if (!isfinite(u)) nf++;
                if (u < tau) lt++;
                else if (u == tau) eq++;
                if (ir[q] < keep) c++;
            }
        }
        if (lt) atomicAdd(&s_L, lt);
        if (eq) atomicAdd(&s_E, eq);
        if (nf) atomicAdd(&s_nf, nf);
        unsigned total;
        unsigned pos = smp_scan(c, s_ws, &total);              // (its barriers: the counts above are complete)
        s.slot = s.b * (size_t)ks.T + (size_t)ti;
        smp_out(a, s, pr, key, (size_t)n, s_nf != 0, (double)s_L, (double)s_E, tau);
        __syncthreads();                                       // every key of this tolerance read before the next one's are written
        if (ti > 0) {
#pragma unroll
            for (int q = 0; q < SM_PER; q++)
                if (ir[q] < keep) {                            // (padding: SM_PAD_ID, never below keep)
                    key[pos] = kr[q];
                    id[pos] = ir[q];
                    pos++;
                }
        }
        __syncthreads();
    }
}

// global path of the tolerance path: grid (P, batch targets); (k0, i0): the segments' sorted entries at a.K = K_max, (k1, i1): the
// other pair of buffers; the tolerances' dense lists alternate between the two
__global__ __launch_bounds__(SM_BS) void k_smp_eval_global(SmArgs a, SmProbs pr, SmKs ks, size_t b0, unsigned long long* k0, unsigned* i0,
                                                           unsigned long long* k1, unsigned* i1) {
    __shared__ unsigned s_ws[SM_BS / 64];
    __shared__ unsigned long long s_L, s_E, s_nf;
    const int t = threadIdx.x, j = (int)blockIdx.x;
    const size_t bl = blockIdx.y, seg = bl * a.P + j;
    SmSeg s = sm_seg(a, b0 + bl, j);
    unsigned long long *ks_ = k0 + seg * a.K, *kd = k1 + seg * a.K;
    unsigned *is = i0 + seg * a.K, *idd = i1 + seg * a.K;
    const double tau = a.cdf ? a.truth[s.b * a.P + s.j] : 0.0;
    for (int ti = ks.T - 1; ti >= 0; ti--) {
        const size_t n = ks.K[ti], keep = ti > 0 ? ks.K[ti - 1] : 0;
        if (t == 0) { s_L = 0; s_E = 0; s_nf = 0; }
        __syncthreads();
        unsigned long long lt = 0, eq = 0, nf = 0;
        size_t carry = 0;
        for (size_t base = 0; base < n; base += SM_TILE) {
            const size_t r0 = base + (size_t)t * SM_PER;
            unsigned long long kr[SM_PER];
            unsigned ir[SM_PER];
            unsigned c = 0;
#pragma unroll
            for (int q = 0; q < SM_PER; q++) {
                const size_t r = r0 + q;
                kr[q] = SM_PAD_KEY;
                ir[q] = SM_PAD_ID;
                if (r < n) {
                    kr[q] = ks_[r];
                    ir[q] = is[r];
                    const double u = sm_unkey(kr[q]);
                    if (!isfinite(u)) nf++;
                    if (u < tau) lt++;
                    else if (u == tau) eq++;
                    if ((size_t)ir[q] < keep) c++;
                }
            }
            if (ti > 0) {                                      // (uniform) the kept entries of the tile, in order, behind the earlier tiles'
                unsigned total;
                size_t pos = carry + smp_scan(c, s_ws, &total);
#pragma unroll
                for (int q = 0; q < SM_PER; q++)
                    if ((size_t)ir[q] < keep) {
                        kd[pos] = kr[q];
                        idd[pos] = ir[q];
                        pos++;
                    }
                carry += total;
            }
        }
        if (lt) atomicAdd(&s_L, lt);
        if (eq) atomicAdd(&s_E, eq);
        if (nf) atomicAdd(&s_nf, nf);
        __syncthreads();
        s.slot = s.b * (size_t)ks.T + (size_t)ti;
        smp_out(a, s, pr, ks_, n, s_nf != 0, (double)s_L, (double)s_E, tau);
        __syncthreads();                                       // (also: the next tolerance's list is written)
        unsigned long long* tk = ks_; ks_ = kd; kd = tk;
        unsigned* tq = is; is = idd; idd = tq;
    }
}

// generic weights: flags[0] |= 1 for a negative or non-finite weight, flags[1] |= 1 for a positive one
__global__ __launch_bounds__(256) void k_sm_wcheck(const double* __restrict__ w, size_t K, int* __restrict__ flags) {
    int neg = 0, pos = 0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < K; e += (size_t)gridDim.x * 256) {
        const double v = w[e];
        if (!(v >= 0.0) || !isfinite(v)) neg = 1;
        else if (v > 0.0) pos = 1;
    }
    if (neg) atomicOr(flags, 1);
    if (pos) atomicOr(flags + 1, 1);
}

// the LDS path up to SM_LDS_MAX (a work-group's sort and knots in 16 K bytes of LDS); diagnostic switch ABC_SUMMARY_PATH=lds / global
// (ABC_DIAG=1) forces a path
bool sm_use_lds(size_t K) {
    if (const char* e = abc_diag_env("ABC_SUMMARY_PATH")) {
        if (!strcmp(e, "lds")) return K <= (size_t)SM_LDS_MAX;
        if (!strcmp(e, "global")) return false;
    }
    return K <= (size_t)SM_LDS_MAX;
}

size_t sm_batch(size_t B, size_t K, size_t P) {
    size_t bb = SM_WS_BYTES / (P * K * 24);
    if (bb < 1) bb = 1;
    if (bb > SM_MAX_GRID_Y) bb = SM_MAX_GRID_Y;
    return bb < B ? bb : B;
}

}  // namespace

size_t abc_summary_need(size_t B, size_t K, size_t P) {
    size_t b = 16 * 256;
    if (!sm_use_lds(K)) {
        const size_t bb = sm_batch(B, K, P), ns = bb * P;
        b += 2 * ns * K * 8 + 2 * ns * K * 4 + 2 * ns * 4 + 8 * 256;
    }
    return b;
}

namespace {

SmProbs sm_probs(const abc_summary* sum) {
    SmProbs pr;
    memset(&pr, 0, sizeof(pr));
    pr.nq = (int)sum->nq;
    for (size_t q = 0; q < sum->nq; q++) pr.q[q] = sum->probs[q];
    return pr;
}

// the B x a.P segments of a.K entries: sort and evaluation; ks: the tolerances of a rejection path (every one evaluated from the one
// sort at a.K = K_max), NULL otherwise; hp: the highest-density intervals in the place of the summary (pr is then not read)
struct HpReq {
    HpMass hm;
    HpOut o;
};
int sm_launch(abc_ctx* ctx, const SmArgs& a, const SmProbs& pr, size_t B, const SmKs* ks, const HpReq* hp = nullptr) {
    const size_t K = a.K, P = (size_t)a.P;
    if (sm_use_lds(K)) {
        int n2 = 1;
        while ((size_t)n2 < K) n2 <<= 1;
        const size_t lds = (size_t)n2 * (ks ? 12 : 16);
        const auto lds_k = a.hcoef ? k_sm_lds<true> : k_sm_lds<false>;
        const auto lds_h = a.hcoef ? k_hp_lds<true> : k_hp_lds<false>;
        ABC_HIP(ctx, hipFuncSetAttribute(hp ? (const void*)lds_h : ks ? (const void*)k_smp_lds : (const void*)lds_k,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        for (size_t b0 = 0; b0 < B; b0 += SM_MAX_GRID_Y) {
            const size_t nb = (B - b0 < SM_MAX_GRID_Y) ? B - b0 : SM_MAX_GRID_Y;
            if (hp) hipLaunchKernelGGL(lds_h, dim3((unsigned)P, (unsigned)nb), dim3(SM_BS), lds, ctx->stream, a, hp->hm, hp->o, n2, b0);
            else if (ks) hipLaunchKernelGGL(k_smp_lds, dim3((unsigned)P, (unsigned)nb), dim3(SM_BS), lds, ctx->stream, a, pr, *ks, n2, b0);
            else hipLaunchKernelGGL(lds_k, dim3((unsigned)P, (unsigned)nb), dim3(SM_BS), lds, ctx->stream, a, pr, n2, b0);
            ABC_HIP(ctx, hipGetLastError());
        }
        return ABC_OK;
    }

    const size_t bb = sm_batch(B, K, P), ns = bb * P;
    unsigned long long* k0 = (unsigned long long*)abc_ws_alloc(ctx, ns * K * 8);
    unsigned long long* k1 = (unsigned long long*)abc_ws_alloc(ctx, ns * K * 8);
    unsigned* i0 = (unsigned*)abc_ws_alloc(ctx, ns * K * 4);
    unsigned* i1 = (unsigned*)abc_ws_alloc(ctx, ns * K * 4);
    unsigned* cnt = (unsigned*)abc_ws_alloc(ctx, ns * 4);
    int* bad = (int*)abc_ws_alloc(ctx, ns * 4);
    if (!k0 || !k1 || !i0 || !i1 || !cnt || !bad) ABC_FAIL(ctx, ABC_ERR_NOMEM, "summary: workspace exhausted");
    double* hpw = nullptr;
    unsigned long long* hpc = nullptr;
    if (hp) {                                                  // the slices' pairs of one batch
        hpw = (double*)abc_ws_alloc(ctx, ns * HP_MAXM * HP_SPLIT * 8);
        hpc = (unsigned long long*)abc_ws_alloc(ctx, ns * HP_MAXM * HP_SPLIT * 8);
        if (!hpw || !hpc) ABC_FAIL(ctx, ABC_ERR_NOMEM, "hpd: workspace exhausted");
    }
    const size_t nch = (K + SM_LDS_MAX - 1) / SM_LDS_MAX;
    const size_t lds_c = (size_t)SM_LDS_MAX * 12;
    const auto chunk_k = a.hcoef ? k_sm_chunk<true> : k_sm_chunk<false>;
    ABC_HIP(ctx, hipFuncSetAttribute((const void*)chunk_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c));
    for (size_t b0 = 0; b0 < B; b0 += bb) {
        const size_t nb = (B - b0 < bb) ? B - b0 : bb, nseg = nb * P, total = nseg * K;
        ABC_HIP(ctx, hipMemsetAsync(cnt, 0, nseg * 4, ctx->stream));
        ABC_HIP(ctx, hipMemsetAsync(bad, 0, nseg * 4, ctx->stream));
        hipLaunchKernelGGL(chunk_k, dim3((unsigned)(nch * P), (unsigned)nb), dim3(SM_BS), lds_c, ctx->stream, a, b0, k0, i0, cnt, bad);
        ABC_HIP(ctx, hipGetLastError());
        unsigned long long *ka = k0, *kb = k1;
        unsigned *ia = i0, *ib = i1;
        size_t blocks = (total + 255) / 256;
        if (blocks > 16384) blocks = 16384;
        for (size_t w = SM_LDS_MAX; w < K; w *= 2) {
            hipLaunchKernelGGL(k_sm_merge, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const unsigned long long*)ka,
                               (const unsigned*)ia, K, total, w, kb, ib);
            ABC_HIP(ctx, hipGetLastError());
            unsigned long long* tk = ka; ka = kb; kb = tk;
            unsigned* ti = ia; ia = ib; ib = ti;
        }
        if (hp) {
            hipLaunchKernelGGL(k_hp_knots_global, dim3((unsigned)P, (unsigned)nb), dim3(SM_BS), 0, ctx->stream, a, b0, (const unsigned*)ia,
                               (double*)kb, (const unsigned*)cnt);
            ABC_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_hp_search_global, dim3((unsigned)(P * HP_SPLIT), (unsigned)nb), dim3(SM_BS), 0, ctx->stream, a, hp->hm,
                               (const unsigned long long*)ka, (const double*)kb, (const unsigned*)cnt, (const int*)bad, hpw, hpc);
            ABC_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_hp_final_global, dim3((unsigned)((nseg * hp->hm.nm + 255) / 256)), dim3(256), 0, ctx->stream, a, hp->hm,
                               hp->o, b0, nseg, (const unsigned long long*)ka, (const double*)kb, (const unsigned*)cnt, (const int*)bad,
                               (const double*)hpw, (const unsigned long long*)hpc);
        } else if (ks)
            hipLaunchKernelGGL(k_smp_eval_global, dim3((unsigned)P, (unsigned)nb), dim3(SM_BS), 0, ctx->stream, a, pr, *ks, b0, ka, ia, kb,
                               ib);
        else
            hipLaunchKernelGGL(k_sm_eval_global, dim3((unsigned)P, (unsigned)nb), dim3(SM_BS), 0, ctx->stream, a, pr, b0,
                               (const unsigned long long*)ka, (const unsigned*)ia, (double*)kb, (const unsigned*)cnt, (const int*)bad);
        ABC_HIP(ctx, hipGetLastError());
    }
    return ABC_OK;
}

}  // namespace

int launch_summary(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const abc_summary* sum) {
    if ((!sum->quant && !sum->cdf) || B == 0 || K == 0 || P == 0) return ABC_OK;
    SmArgs a = sm_args(sv, K, P);
    a.truth = sum->truth;
    a.quant = sum->quant;
    a.cdf = sum->cdf;
    return sm_launch(ctx, a, sm_probs(sum), B, nullptr);
}

// the summary's sort, buffers and batches (the knots lie in the spare key buffer), and on the global path the slices' pairs
size_t abc_hpd_need(size_t B, size_t K, size_t P) {
    size_t b = abc_summary_need(B, K, P);
    if (!sm_use_lds(K)) b += 2 * sm_batch(B, K, P) * P * HP_MAXM * HP_SPLIT * 8 + 2 * 256;
    return b;
}

int launch_hpd(abc_ctx* ctx, const SmValues& sv, size_t B, size_t K, size_t P, const abc_hpd* hd) {
    if (B == 0 || K == 0 || P == 0) return ABC_OK;
    const SmArgs a = sm_args(sv, K, P);
    HpReq hp;
    memset(&hp, 0, sizeof(hp));
    hp.hm.nm = (int)hd->nm;
    for (size_t i = 0; i < hd->nm; i++) hp.hm.m[i] = hd->mass[i];
    hp.o = HpOut{hd->lo, hd->hi, hd->plo, hd->phi};
    SmProbs pr;
    memset(&pr, 0, sizeof(pr));
    return sm_launch(ctx, a, pr, B, nullptr, &hp);
}

size_t abc_path_summary_need(size_t B, const size_t* Ks, size_t T, size_t P, int method) {
    if (method == 0) return abc_summary_need(B, Ks[T - 1], P);       // the one sort at K_max
    size_t b = 0;
    for (size_t t = 0; t < T; t++) {                                 // one tolerance's launch set at a time
        const size_t bt = abc_summary_need(B, Ks[t], P);
        if (bt > b) b = bt;
    }
    return b;
}

int launch_path_summary(abc_ctx* ctx, const SmValues& sv, size_t B, const size_t* Ks, size_t T, size_t P, const abc_summary* sum) {
    if ((!sum->quant && !sum->cdf) || B == 0 || P == 0) return ABC_OK;
    SmArgs a = sm_args(sv, Ks[T - 1], P);                            // ld = K_max
    a.truth = sum->truth;
    a.quant = sum->quant;
    a.cdf = sum->cdf;
    a.T = (int)T;
    const SmProbs pr = sm_probs(sum);
    // under row importance weights the rejection path's segments are weighted too: the one-sort unit-weight walk does not apply,
    // and every tolerance goes through the general kernels with K = K_t, as the loclinear path (slot (b, t) = the summary call at K_t)
    if (sv.method == 0 && !sv.om) {
        SmKs ks = {};
        ks.T = (int)T;
        for (size_t t = 0; t < T; t++) ks.K[t] = Ks[t];
        a.t = (int)T - 1;
        return sm_launch(ctx, a, pr, B, &ks);
    }
    for (size_t t = 0; t < T; t++) {
        a.K = Ks[t];
        a.t = (int)t;
        const size_t mark = ctx->ws_off;                             // (stream order: a tolerance's buffers are free for the next)
        ABC_TRY(sm_launch(ctx, a, pr, B, nullptr));
        ctx->ws_off = mark;
    }
    return ABC_OK;
}

int abc_summary_check_weights(abc_ctx* ctx, const double* w, size_t K, const char* fn) {
    int* flags = (int*)abc_ws_alloc(ctx, 2 * sizeof(int));
    if (!flags) ABC_FAIL(ctx, ABC_ERR_NOMEM, "%s: workspace exhausted", fn);
    ABC_HIP(ctx, hipMemsetAsync(flags, 0, 2 * sizeof(int), ctx->stream));
    size_t blocks = (K + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_sm_wcheck, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, w, K, flags);
    ABC_HIP(ctx, hipGetLastError());
    int h[2] = {0, 0};
    ABC_HIP(ctx, hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    ABC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h[0]) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: a weight is negative or non-finite", fn);
    if (!h[1]) ABC_FAIL(ctx, ABC_ERR_INVALID, "%s: every weight is zero", fn);
    return ABC_OK;
}

static_assert(SM_TILE == SM_LDS_MAX, "the LDS path evaluates its segment in one tile");
