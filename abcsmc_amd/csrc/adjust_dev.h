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

// theta*_e[j] = theta_e[j] - sum_k beta_kj x_e[k]: one fma chain in k order; x(k) = x_e[k] (observation-centred score),
// beta[k ldb] = beta_kj
template <class XF>
__device__ __forceinline__ double aj_adjusted(double th, XF x, const double* beta, size_t ldb, int nc) {
    double a = th;
#pragma unroll 8
    for (int k = 0; k < nc; k++) a = fma(-beta[(size_t)k * ldb], x(k), a);
    return a;
}

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
};
