// Parameter transforms of the local-linear adjustment (abc_ctx_set_param_transf; the definition is in the header).  Every kernel
// that transforms calls these functions, so a value has the same bits wherever it is made: the forward pass (k_tf_apply), the
// adjusted rows (k_adj_apply) and the segments' values (sm_value).  Every operation is written out; nothing here is an expression
// the compiler may contract differently at two sites.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

// device copies of the context's setting (uploaded at set time); kind == NULL: no transform
struct AbcTf {
    const int32_t* kind;    // P entries: ABC_TRANSF_NONE / LOG / LOGIT (0 / 1 / 2)
    const double* lo;       // P entries, read for LOGIT only
    const double* hi;
};

// t = log(y) for finite y > 0, otherwise NaN (y == 0 too)
__device__ __forceinline__ double tf_fwd_log(double y) {
    if (!(y > 0.0) || isinf(y)) return __builtin_nan("");
    return log(y);
}
// t = log((y - lo) / (hi - y)) for lo < y < hi, otherwise NaN
__device__ __forceinline__ double tf_fwd_logit(double y, double lo, double hi) {
    if (!(y > lo) || !(y < hi)) return __builtin_nan("");
    const double a = y - lo;
    const double b = hi - y;
    const double r = a / b;
    return log(r);
}
__device__ __forceinline__ double tf_back_log(double t) {
    if (isnan(t)) return t;
    return exp(t);
}
// s = 1 / (1 + exp(-t)), y = fma(hi - lo, s, lo), clamped to [lo, hi]; NaN stays NaN (tested first: fmin / fmax would drop it)
__device__ __forceinline__ double tf_back_logit(double t, double lo, double hi) {
    if (isnan(t)) return t;
    const double e = exp(-t);
    const double d = 1.0 + e;
    const double s = 1.0 / d;
    const double w = hi - lo;
    double y = fma(w, s, lo);
    if (y < lo) y = lo;
    if (y > hi) y = hi;
    return y;
}

// kind 0: the value itself, bit for bit
__device__ __forceinline__ double tf_forward(int kind, double lo, double hi, double y) {
    if (kind == 1) return tf_fwd_log(y);
    if (kind == 2) return tf_fwd_logit(y, lo, hi);
    return y;
}
__device__ __forceinline__ double tf_back(int kind, double lo, double hi, double t) {
    if (kind == 1) return tf_back_log(t);
    if (kind == 2) return tf_back_logit(t, lo, hi);
    return t;
}
// parameter j of a setting (tf.kind != NULL)
__device__ __forceinline__ double tf_back_j(const AbcTf& tf, int j, double t) {
    const int kind = tf.kind[j];
    if (kind == 0) return t;
    return tf_back(kind, kind == 2 ? tf.lo[j] : 0.0, kind == 2 ? tf.hi[j] : 0.0, t);
}
