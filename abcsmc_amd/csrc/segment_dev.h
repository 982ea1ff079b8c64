// How a segment's values and weights are made, shared by summary.hip and density.hip.  A segment is one (target b, parameter j):
// K values made in registers from the ranking's rows (Y, or the adjusted value theta* of adjust_dev.h, which k_adj_apply computes
// with the same function), or read from a given matrix.  Both files call these functions, so the quantiles and the densities of
// a segment see the same bits.
#pragma once
#include <string.h>

#include "abc_internal.h"
#include "adjust_dev.h"

// what a kernel needs to make the values and weights of segment (b0 + blockIdx.y, j); the last three members are the
// summaries' own inputs and outputs (summary.hip), NULL elsewhere
struct SmArgs {
    int method;                 // 0 rejection, 1 loclinear, 2 generic
    const uint64_t* idx;        // B rows of ld entries, the first K of a row are the segment's
    const double* Y;
    size_t ldy;
    AjSrc src;                  // method 1: as launch_rank_targets_adjust read the rows
    const double* O;
    int KCO, nc, A, P, kernel;
    const double* coef;
    const double* dist;
    AbcTf tf;                   // method 1: the fit's parameter transforms (kind == NULL: none)
    const double* hcoef;        // method 1: the variance correction's second fit, laid out as coef (NULL: off)
    const double* V;            // method 2
    size_t ldv;
    const double* w;
    const double* om;           // methods 0 and 1: row importance weights (NULL: none), the weight of entry e times om[idx[e]]
    size_t K;                   // entries of a segment (a tolerance path: K_t)
    size_t ld;                  // row stride of idx and dist (K; a tolerance path: K_max)
    int T, t;                   // tolerance t of T (1, 0 outside a path): coefficients and outputs at slot b T + t
    const double* truth;        // B x P (device)
    double* quant;              // B x T x nq x P
    double* cdf;                // B x T x P
};

struct SmSeg {
    size_t b;
    size_t slot;                // b T + t: where the segment's coefficients and outputs are
    int j;
    const uint64_t* ix;
    const double* dd;
    double h;
    bool rect;
    const double* beta;         // method 1: beta_kj at beta[k P]
    const double* ob;           // method 1: the target's scores
    const double* g;            // method 1 under the variance correction: g_kj at g[k P]; NULL: off, or this parameter is skipped
    double alpha;               // ... and the first fit's intercept
};

// the value-making members of SmArgs from a caller's SmValues (host)
static inline SmArgs sm_args(const SmValues& sv, size_t K, size_t P) {
    SmArgs a;
    memset(&a, 0, sizeof(a));
    a.method = sv.method;
    a.idx = sv.idx;
    a.Y = sv.Y;
    a.ldy = sv.ldy;
    a.A = sv.A;
    a.P = (int)P;
    a.kernel = sv.kernel;
    if (sv.method == 1) {
        a.src = sv.adj->src;
        a.O = sv.adj->O;
        a.KCO = sv.adj->KCO;
        a.nc = sv.adj->nc;
        a.coef = sv.adj->coef;
        a.dist = sv.adj->dist;
        a.tf = sv.adj->tf;
        a.hcoef = sv.adj->hcoef;
    }
    a.V = sv.V;
    a.ldv = sv.ldv;
    a.w = sv.w;
    a.om = sv.method == 2 ? nullptr : sv.om;
    a.K = K;
    a.ld = K;
    a.T = 1;
    a.t = 0;
    return a;
}

// the variance correction's members of a method-1 segment whose slot, j and beta are set: g stays NULL for a skipped parameter
__device__ __forceinline__ void sm_seg_hc(const SmArgs& a, SmSeg& s) {
    const double* hc = a.hcoef + s.slot * (size_t)(a.A + 1) * a.P + s.j;
    s.g = nullptr;
    s.alpha = 0.0;
    if (!isnan(hc[0])) {
        s.g = hc + a.P;
        s.alpha = s.beta[-(ptrdiff_t)a.P];
    }
}

// HC: with the variance correction's members (the instances that make corrected values)
template <bool HC = false>
__device__ __forceinline__ SmSeg sm_seg(const SmArgs& a, size_t b, int j) {
    SmSeg s;
    s.b = b;
    s.slot = b * (size_t)a.T + (size_t)a.t;
    s.j = j;
    s.ix = a.idx ? a.idx + b * a.ld : nullptr;
    s.dd = nullptr;
    s.h = 0.0;
    s.rect = true;
    s.beta = nullptr;
    s.ob = nullptr;
    s.g = nullptr;
    s.alpha = 0.0;
    if (a.method == 1) {
        s.dd = a.dist + b * a.ld;
        s.h = s.dd[a.K - 1];
        s.rect = a.kernel == 1 || aj_fallback(s.dd, a.K);
        s.beta = a.coef + s.slot * (size_t)(a.A + 1) * a.P + a.P + j;
        s.ob = a.O + b * (size_t)a.KCO;
        if constexpr (HC) sm_seg_hc(a, s);
    }
    return s;
}

// TF = false: an instance without the back-transform for a kernel whose registers it would cost (its launcher takes it when
// a.tf.kind == NULL, so calls without transforms run the code they ran before there were any).  HC = true: the instance with the
// variance correction (aj_hcorr, as k_adj_apply), which a launcher takes only when a.hcoef is set, for the same reason.
template <bool TF = true, bool HC = false>
__device__ __forceinline__ double sm_value(const SmArgs& a, const SmSeg& s, size_t e) {
    if (a.method == 0) return a.Y[(size_t)s.ix[e] + a.ldy * (size_t)s.j];
    if (a.method == 1) {
        const size_t i = (size_t)s.ix[e];
        const int nc = a.nc;
        const auto x = [&](int k) { return aj_val(a.src, i, k, nc) - s.ob[k]; };
        double v = aj_adjusted(aj_val(a.src, i, nc + s.j, nc), x, s.beta, (size_t)a.P, nc);
        if constexpr (HC)
            if (s.g) v = aj_hcorr(v, s.alpha, x, s.g, (size_t)a.P, nc);
        if constexpr (TF) return a.tf.kind ? tf_back_j(a.tf, s.j, v) : v;     // (the fit's scale back to the parameter's own)
        return v;
    }
    return a.V[e + a.ldv * (size_t)s.j];
}

// under row importance weights (a.om, methods 0 and 1) the weight is k_e om[i_e], the product abc_adjust_out.weight holds (under
// method 0 k_e = 1, so the bits of om[i_e]); a.om is a kernel argument, uniform over the launch, as a.method and a.w are
__device__ __forceinline__ double sm_weight(const SmArgs& a, const SmSeg& s, size_t e) {
    if (a.method == 2) return a.w ? a.w[e] : 1.0;
    const double k = (a.method == 1) ? aj_weight(s.dd[e], s.h, s.rect) : 1.0;
    return a.om ? k * a.om[(size_t)s.ix[e]] : k;
}
