// The Philox4x32-10 counter generator and the four normal deviates made of one of its blocks: the device noise stream of the
// proposals (resample.hip) and of the posterior draws (draws.hip).  Both files call these functions, so a block means the same
// deviates in both; tests/_philox_ref.py is their NumPy model.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- Philox4x32-10 --------------------------------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}
// FOUR independent N(0,1) from one Philox block: two Box-Muller pairs on the f32 transcendental hardware (v_log_f32,
// v_sqrt_f32, v_sin_f32 / v_cos_f32, 8 issue cycles each) instead of double-precision library calls -- the fp64 log, sqrt and
// sincospi of round 1 were ~300 vector instructions per pair and made the noise kernels compute-bound (71 us for 1.6e7
// deviates); this is ~20 per pair plus half a Philox block.  The radius comes from all 32 bits of its word,
//   -2 ln u = -2 ln 2 (log2(r + 1/2) - 32),   u in [2^-33, 1):  |z| <= 6.76,
// (the conversion of r to f32 rounds at 6e-8 relative: 9e-8 absolute in the logarithm), the angle from the top 24 bits of
// its word, in revolutions (what v_sin_f32 / v_cos_f32 take).  The deviates carry f32 rounding (~1e-7 relative): the device
// noise stream is distributional by contract (declared deviations); the reference-stream mode is untouched.
__device__ __forceinline__ void normal4(U4 r, double (&z)[4]) {
    const float NEG2LN2 = -1.3862943611198906f;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t ru = h ? r.z : r.x, ra = h ? r.w : r.y;
        const float lg = __builtin_amdgcn_logf((float)ru + 0.5f) - 32.0f;           // log2 u, in [-33, 0)
        const float rad = __builtin_amdgcn_sqrtf(__builtin_fmaxf(NEG2LN2 * lg, 0.0f));   // (v_log_f32 may return 32 + 1 ulp at the top)
        const float ang = (float)(ra >> 8) * 5.9604644775390625e-08f;             // [0, 1) revolutions, exact
        z[2 * h] = (double)(rad * __builtin_amdgcn_cosf(ang));
        z[2 * h + 1] = (double)(rad * __builtin_amdgcn_sinf(ang));
    }
}
