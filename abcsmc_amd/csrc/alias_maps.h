// The step-map algebra of the device alias build (alias_dev.hip; the family and why it is closed under composition are described
// in that file's header and in scripts/alias_scan_proto.py).  Plain 128-bit integer arithmetic, the same on the host and on the
// device: the kernels include this header, and tests/cxx/alias_maps_probe.cpp holds every function against brute force on the CPU
// (also under the address and undefined-behaviour sanitizers: the shifts, the ceilings of negative operands).
#pragma once
#include <math.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ABC_AL_HD __host__ __device__ __forceinline__
#else
#define ABC_AL_HD inline
#endif

namespace abc_al {

typedef __int128 i128;
typedef unsigned __int128 u128;
typedef unsigned long long u64;

struct RMap { i128 t0, t1, b; int k; int pad_[3]; };      // 64 bytes

ABC_AL_HD int al_clz64(u64 v) {                           // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}
ABC_AL_HD u64 al_double_bits(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (u64)__double_as_longlong(x);
#else
    u64 b;
    memcpy(&b, &x, sizeof b);
    return b;
#endif
}

ABC_AL_HD i128 shl(i128 v, int s) { return (i128)((u128)v << s); }
ABC_AL_HD int bitlen(i128 v) {                            // v >= 0
    const u64 hi = (u64)((u128)v >> 64), lo = (u64)v;
    return hi ? 128 - al_clz64(hi) : (lo ? 64 - al_clz64(lo) : 0);
}
ABC_AL_HD int level_of(i128 v) { const int b = bitlen(v); return b > 53 ? b - 53 : 0; }

// y -> round-to-nearest-even at level k of (y + c); sticky: c stands for a real number slightly above the integer c
ABC_AL_HD RMap rne_map(int k, i128 c, bool sticky) {
    RMap m;
    m.k = k; m.b = 0; m.pad_[0] = m.pad_[1] = m.pad_[2] = 0;
    if (k == 0) { m.t0 = -c - 1; m.t1 = -c; return m; }
    const i128 P = shl(1, k + 1), h = shl(1, k - 1);
    const i128 t_even = -c - shl(1, k) + h;                // reaching an EVEN multiple of 2^k: a tie rounds up to it
    const i128 t_odd = -c + h + (sticky ? 0 : 1);          // reaching an ODD multiple: a tie stays below
    m.t0 = t_odd - P; m.t1 = t_even;
    return m;
}
ABC_AL_HD RMap rmap_identity() { RMap m; m.k = 0; m.t0 = -1; m.t1 = 0; m.b = 0; m.pad_[0] = m.pad_[1] = m.pad_[2] = 0; return m; }
ABC_AL_HD i128 rapply(const RMap& m, i128 y) {
    return shl(((y - m.t0) >> (m.k + 1)) + ((y - m.t1) >> (m.k + 1)), m.k) + m.b;
}
// min { y : m(y) >= v }
ABC_AL_HD i128 inv_min(const RMap& m, i128 v) {
    const i128 a = -((-(v - m.b)) >> m.k);                 // ceil((v - b) / 2^k): the step count that must be reached
    if (a & 1) return m.t0 + shl((a + 1) >> 1, m.k + 1);
    return m.t1 + shl(a >> 1, m.k + 1);
}
// first m1, then m2
ABC_AL_HD RMap compose(const RMap& m1, const RMap& m2) {
    RMap r;
    if (m2.k < m1.k) { r = m1; r.b = rapply(m2, m1.b); return r; }     // 2^k1 N is a multiple of m2's period
    r.k = m2.k; r.t0 = inv_min(m1, m2.t0); r.t1 = inv_min(m1, m2.t1); r.b = m2.b;
    r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
    return r;
}

// x (>= 0, finite) as an integer multiple of 2^e0; *inexact is set when bits fall below the grid (the result is then the floor)
ABC_AL_HD i128 to_grid(double x, int e0, bool* inexact) {
    const u64 bits = al_double_bits(x);
    const int be = (int)((bits >> 52) & 0x7ff);
    u64 mant = bits & 0xfffffffffffffull;
    int e;
    if (be == 0) { if (mant == 0) return 0; e = -1074; } else { mant |= 1ull << 52; e = be - 1075; }
    const int sh = e - e0;
    if (sh >= 0) return (sh < 70) ? shl((i128)mant, sh) : (i128)0;       // (sh >= 70 cannot happen for values the callers admit)
    if (sh <= -64) { *inexact = true; return 0; }
    if (mant & ((1ull << -sh) - 1)) *inexact = true;
    return (i128)(mant >> -sh);
}
// the double with value v 2^e0, if v has at most 53 significant bits (else *ok = false)
ABC_AL_HD double from_grid(i128 v, int e0, bool* ok) {
    if (v < 0) { *ok = false; return 0.0; }
    if (v == 0) return 0.0;
    const int bl = bitlen(v), sh = bl > 53 ? bl - 53 : 0;
    const u64 top = (u64)(v >> sh);
    if (shl((i128)top, sh) != v) { *ok = false; return 0.0; }
    return ldexp((double)top, sh + e0);
}

}  // namespace abc_al
