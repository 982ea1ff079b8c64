// What the marginal densities (density.hip) and the pair densities (joint.hip) share on the device: a segment's bandwidth, grid and
// kernel constants as k_dn_moments makes them, and the evaluation of the Gaussian kernel.  Both files call dn_kern, so a factor of
// a pair density is formed exactly as a term of the marginal one.
#pragma once
#include <math.h>

struct DnSeg {                                              // per segment, made by k_dn_moments (all NaN: a bad segment)
    double h, lo_x, step, den, c;                           // den = W h sqrt(2 pi), c = sqrt(log2(e) / 2) / h
};

__device__ __forceinline__ double dn_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// 2^-(z^2); below 2^-2000 it is 0 either way
__device__ __forceinline__ double dn_kern(double z) {
    const double t = fmax(-(z * z), -2000.0);
#ifdef DN_EXP_FP64
    return exp2(t);
#else
    const double n = rint(t);
    const float p = __builtin_amdgcn_exp2f((float)(t - n));
    return ldexp((double)p, (int)n);
#endif
}
