// Device pieces of the local-linear adjustment shared by adjust.hip and summary.hip: where the retained rows are read from,
// the kernel weights and the adjusted value theta*.  Both files call the same functions, so the summaries of the adjusted rows
// see the bits that abc_adjust_out.theta / .weight hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "transf_dev.h"

// where the retained rows are read from: the table (T != NULL, row i at T + i W) or the scores and Y directly (same bits)
struct AjSrc {
    const double* T;
    size_t W;
    const double* S;
    size_t sld;
    const double* Y;
    size_t ldy;
};

__device__ __forceinline__ double aj_val(const AjSrc& s, size_t i, int c, int nc) {
    if (s.T) return s.T[i * s.W + (size_t)c];
    return (c < nc) ? s.S[i + s.sld * (size_t)c] : s.Y[i + s.ldy * (size_t)(c - nc)];
}

// chunks of a target's K retained rows for the chunked moment passes (adjust.hip, glm.hip): about 256 rows each, 64 chunks at
// most; from K alone, so that a target's sums do not depend on the batch or on the fit
struct AjChunks {
    size_t nch, CH;          // chunks and their size
};
static inline AjChunks aj_chunks(size_t K) {
    AjChunks p;
    p.nch = (K + 255) / 256;
    if (p.nch > 64) p.nch = 64;
    p.CH = (K + p.nch - 1) / p.nch;
    p.nch = (K + p.CH - 1) / p.CH;
    return p;
}

// the Epanechnikov weights of a target are all 0 exactly when its first one is (d ascending, w non-increasing in d)
__device__ __forceinline__ bool aj_fallback(const double* d, size_t K) {
    const double h = d[K - 1];
    if (h == 0.0) return true;
    const double t = d[0] / h;
    return 1.0 - t * t == 0.0;
}
__device__ __forceinline__ double aj_weight(double de, double h, bool rect) {
    if (rect) return 1.0;
    const double t = de / h;
    return 1.0 - t * t;
}

// ---- row importance weights (abc_ctx_set_row_weights; the definition is in the header) ----
// w_e = k_e omega[i_e], one fp64 multiplication, in the RW instances only: the others never see omega
template <bool RW>
__device__ __forceinline__ double aj_weight_rw(double de, double h, bool rect, const double* __restrict__ om, size_t i) {
    const double k = aj_weight(de, h, rect);
    if constexpr (RW) return k * om[i];
    return k;
}

// theta*_e[j] = theta_e[j] - sum_k beta_kj x_e[k]: one fma chain in k order; x(k) = x_e[k] (observation-centred score),
// beta[k ldb] = beta_kj
template <class XF>
__device__ __forceinline__ double aj_adjusted(double th, XF x, const double* beta, size_t ldb, int nc) {
    double a = th;
#pragma unroll 8
    for (int k = 0; k < nc; k++) a = fma(-beta[(size_t)k * ldb], x(k), a);
    return a;
}

// ---- heteroscedastic variance correction (abc_ctx_set_adjust_hcorr; the definition is in the header) ----
// the corrected value of a row: v the plain adjusted value (aj_adjusted's bits), alpha the stored intercept, g[k ldb] = g_kj the
// second fit's slopes; r = v - alpha, q = sum_k g_kj x_e[k] (one fma chain from 0.0 in k order), theta** = fma(r, exp(-q / 2), alpha)
template <class XF>
__device__ __forceinline__ double aj_hcorr(double v, double alpha, XF x, const double* g, size_t ldb, int nc) {
    double q = 0.0;
#pragma unroll 8
    for (int k = 0; k < nc; k++) q = fma(g[(size_t)k * ldb], x(k), q);
    return fma(v - alpha, exp(-0.5 * q), alpha);
}
// the second fit's response of a row: z = 2 log|v - alpha| (-inf for a zero residual, NaN or +inf for a non-finite one)
__device__ __forceinline__ double aj_logres(double v, double alpha) { return 2.0 * log(fabs(v - alpha)); }

// where a regressing call under the correction writes the second fit (the context's record) and counts the skipped parameters
struct AbcHc {
    double* hcoef;                  // slots x (A + 1) x P, laid out as coef; NULL: the correction is off
    unsigned long long* skipped;    // device counter
};

// ---- ridge adjustment (abc_ctx_set_adjust_ridge; the definition is in the header) ----
// the penalties of a regressing call under the setting and where it writes its record (the context's buffers)
struct AbcRg {
    double lambda[8];               // ascending (ABC_RIDGE_MAXL entries at most)
    int L;                          // 0: the setting is off
    int32_t* pick;                  // slots x P: the chosen penalty's index
    double* press;                  // slots x L x P: the leave-one-out PRESS of every penalty
    unsigned long long* unscored;   // device counter: (slot, parameter) pairs with every penalty's PRESS +inf
};

// what launch_rank_targets_adjust leaves in the arena for a caller that reads the adjusted rows itself (summary.hip)
struct abc_adj_keep {
    AjSrc src;
    const double* O;        // targets' scores, O[b KCO + k]
    int KCO;
    int nc;
    const double* coef;     // B x (A + 1) x P
    const double* dist;     // B x K
    AbcTf tf;               // the parameter transforms the fit was made under (kind == NULL: none): src.Y is forward(Y), and a reader
                            // of the adjusted rows carries theta* back with tf_back_j
    const double* hcoef;    // the variance correction's second fit, laid out as coef (NULL: off); a NaN in row 0 of a parameter:
                            // skipped, the row is the plain adjusted value
};
