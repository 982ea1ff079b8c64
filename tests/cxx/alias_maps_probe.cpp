// Host probe of abcsmc_amd/csrc/alias_maps.h, the step-map algebra of the device alias build (alias_dev.hip): every function
// against brute force in __int128.
//   1. rapply(rne_map(k, c, sticky), y) is round-to-nearest-even of y + c at level k (sticky: of y + c + 1/2): k = 0..6 over two
//      periods of y and a window of c, both signs; k up to 70 on random operands
//   2. inv_min(m, v) is the least y with m(y) >= v: small k exhaustively, and over random chains of maps
//   3. compose: chains of 2..64 maps of mixed levels applied one after another against the composed map (folded from the left,
//      from the right and as a tree: associativity), over a window of y and random y
//   4. to_grid / from_grid: round trip of doubles on the grid (subnormals, zero, sh = -63, -64, 0, 69), `inexact` exactly when
//      bits fall below the grid, `ok = false` exactly when the value has more than 53 significant bits
// Prints "ok <cases>" or the first counter-example (exit status 1).
//   g++ -O2 -std=c++17 tests/cxx/alias_maps_probe.cpp -o probe && ./probe        (also with -fsanitize=address,undefined)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "../../abcsmc_amd/csrc/alias_maps.h"

using namespace abc_al;

static long long g_cases = 0;

static std::string str(i128 v) {
    if (v == 0) return "0";
    const bool neg = v < 0;
    u128 u = neg ? (u128)0 - (u128)v : (u128)v;
    std::string s;
    while (u) { s.insert(s.begin(), (char)('0' + (int)(u % 10))); u /= 10; }
    return neg ? "-" + s : s;
}
static std::string str(const RMap& m) { return "{k=" + std::to_string(m.k) + " t0=" + str(m.t0) + " t1=" + str(m.t1) + " b=" + str(m.b) + "}"; }
[[noreturn]] static void fail(const std::string& what) {
    printf("FAIL %s\n", what.c_str());
    exit(1);
}

static std::mt19937_64 g_rng(20240607);
static u64 rnd() { return g_rng(); }
static int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (u64)(hi - lo + 1)); }
// uniform in (-2^bits, 2^bits), bits <= 126
static i128 rnd_signed(int bits) {
    u128 u = ((u128)rnd() << 64) | rnd();
    if (bits < 128) u &= (((u128)1) << bits) - 1;
    const i128 v = (i128)u;
    return (rnd() & 1) ? -v : v;
}

// brute force: floor division by 2^k without relying on the shift of a negative number
static i128 floor_div_pow2(i128 x, int k) {
    const i128 d = (i128)1 << k;
    i128 q = x / d;                        // truncates towards zero
    if (x % d != 0 && x < 0) q -= 1;
    return q;
}
// round x (sticky: x + 1/2) to the nearest multiple of 2^k, ties to the even multiple
static i128 rne_brute(i128 x, int k, bool sticky) {
    if (k == 0) return x;
    const i128 d = (i128)1 << k, half = d / 2;
    const i128 q = floor_div_pow2(x, k), r = x - q * d;
    bool up;
    if (sticky) up = r >= half;            // r + 1/2 against half: never a tie
    else if (r != half) up = r > half;
    else up = (q % 2) != 0;                // a tie: to the even multiple
    return (q + (up ? 1 : 0)) * d;
}

// ------------------------------------------------------------------------------------------------------------------------ 1.
static void check_rne_one(int k, i128 c, bool sticky, i128 y) {
    const RMap m = rne_map(k, c, sticky);
    const i128 got = rapply(m, y), want = rne_brute(y + c, k, sticky);
    g_cases++;
    if (got != want)
        fail("rne: k=" + std::to_string(k) + " c=" + str(c) + " sticky=" + std::to_string((int)sticky) + " y=" + str(y) + ": rapply " +
             str(got) + ", brute force " + str(want));
    if (!(m.t0 <= m.t1 && m.t1 <= m.t0 + ((i128)1 << (k + 1)))) fail("rne: thresholds out of order " + str(m));
}
static void check_rne() {
    for (int k = 0; k <= 6; k++) {
        const int P = 1 << (k + 1);
        for (int sticky = 0; sticky <= (k ? 1 : 0); sticky++)          // (level 0 has no bits below it: the kernels refuse a sticky operand there)
            for (int c = -3 * P - 5; c <= 3 * P + 5; c++)
                for (int y = -P - 3; y <= P + 3; y++) check_rne_one(k, c, sticky != 0, y);
    }
    for (int it = 0; it < 200000; it++) {
        const int k = rnd_int(0, 70);
        const bool sticky = k && (rnd() & 1);
        // operands as the chains hold them (a value of up to 53 bits above level k) and a few bits beyond, both signs
        i128 y = rnd_signed(rnd_int(1, k + 54)), c = rnd_signed(rnd_int(1, k + 54));
        if (k && (it & 3) == 0) {          // land on or next to a tie
            const i128 d = (i128)1 << k;
            y = floor_div_pow2(y + c, k) * d + d / 2 - c + rnd_int(-1, 1);
        }
        check_rne_one(k, c, sticky, y);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ 2.
static void check_inv_one(const RMap& m, i128 v) {
    const i128 y = inv_min(m, v);
    g_cases++;
    if (!(rapply(m, y) >= v) || !(rapply(m, y - 1) < v))
        fail("inv_min: m=" + str(m) + " v=" + str(v) + ": y=" + str(y) + " m(y)=" + str(rapply(m, y)) + " m(y-1)=" + str(rapply(m, y - 1)));
}
static RMap random_map(int kmax, int cbits_over_k) {
    const int k = rnd_int(0, kmax);
    const bool sticky = k && (rnd() & 1);
    return rne_map(k, rnd_signed(rnd_int(1, k + cbits_over_k)), sticky);
}
static void check_inv_min() {
    for (int k = 0; k <= 5; k++) {
        const int P = 1 << (k + 1);
        for (int sticky = 0; sticky <= (k ? 1 : 0); sticky++)
            for (int c = -P - 2; c <= P + 2; c++)
                for (int b = -3; b <= 3; b++) {
                    RMap m = rne_map(k, c, sticky != 0);
                    m.b = b;
                    // monotone over the window (what makes the two-point test below a proof of "least")
                    for (int y = -3 * P; y < 3 * P; y++)
                        if (rapply(m, y) > rapply(m, y + 1)) fail("map not monotone: " + str(m) + " at y=" + str(y));
                    for (int v = -3 * P; v <= 3 * P; v++) {
                        check_inv_one(m, v);
                        // ... and literally the least, by search
                        const i128 y = inv_min(m, v);
                        i128 z = y - 2 * P - 8;
                        while (rapply(m, z) < v) z++;
                        if (z != y) fail("inv_min: m=" + str(m) + " v=" + str(v) + ": " + str(y) + ", search " + str(z));
                    }
                }
    }
    for (int it = 0; it < 20000; it++) {
        const int n = rnd_int(1, 24);
        RMap m = random_map(60, 50);
        for (int j = 1; j < n; j++) m = compose(m, random_map(60, 50));
        check_inv_one(m, rnd_signed(rnd_int(1, 114)));
        check_inv_one(m, rapply(m, rnd_signed(100)) + rnd_int(-2, 2));
    }
}

// ------------------------------------------------------------------------------------------------------------------------ 3.
static RMap fold_left(const std::vector<RMap>& ms, size_t lo, size_t hi) {
    RMap m = ms[lo];
    for (size_t j = lo + 1; j < hi; j++) m = compose(m, ms[j]);
    return m;
}
static RMap fold_right(const std::vector<RMap>& ms, size_t lo, size_t hi) {
    RMap m = ms[hi - 1];
    for (size_t j = hi - 1; j-- > lo;) m = compose(ms[j], m);
    return m;
}
static RMap fold_tree(const std::vector<RMap>& ms, size_t lo, size_t hi) {
    if (hi - lo == 1) return ms[lo];
    const size_t mid = lo + (hi - lo + 1) / 2;
    return compose(fold_tree(ms, lo, mid), fold_tree(ms, mid, hi));
}
static void check_compose_at(const std::vector<RMap>& ms, const RMap& l, const RMap& r, const RMap& t, const RMap& split, i128 y) {
    i128 x = y;
    for (const RMap& m : ms) x = rapply(m, x);
    const i128 a = rapply(l, y), b = rapply(r, y), c = rapply(t, y), d = rapply(split, y);
    g_cases++;
    if (a != x || b != x || c != x || d != x)
        fail("compose: chain of " + std::to_string(ms.size()) + " maps at y=" + str(y) + ": one after another " + str(x) + ", left fold " + str(a) +
             ", right fold " + str(b) + ", tree " + str(c) + ", (a.b).c at a random split " + str(d) + "; first maps " + str(ms[0]) + " " + str(ms[1]));
}
static void check_compose() {
    bool saw_down = false, saw_up = false;
    for (int it = 0; it < 6000; it++) {
        const int n = rnd_int(2, 64);
        // a third of the chains at small levels (windows of y cross many steps), a third at levels as the kernels meet them
        // (neighbouring binades), a third anywhere up to 60
        const int mode = it % 3;
        std::vector<RMap> ms;
        const int kbase = mode == 1 ? rnd_int(0, 58) : 0;
        for (int j = 0; j < n; j++) {
            RMap m;
            if (mode == 0) m = random_map(4, 4);
            else if (mode == 1) { const int k = kbase + rnd_int(0, 2); m = rne_map(k, rnd_signed(rnd_int(1, k + 52)), k && (rnd() & 1)); }
            else m = random_map(60, 50);
            if (j && m.k < ms.back().k) saw_down = true;
            if (j && m.k > ms.back().k) saw_up = true;
            ms.push_back(m);
        }
        const RMap l = fold_left(ms, 0, n), r = fold_right(ms, 0, n), t = fold_tree(ms, 0, n);
        // (a.b).c and a.(b.c) with a, b, c themselves chains
        RMap split = l;
        if (n >= 3) {
            const size_t i1 = (size_t)rnd_int(1, n - 2), i2 = (size_t)rnd_int((int)i1 + 1, n - 1);
            const RMap a = fold_left(ms, 0, i1), b = fold_tree(ms, i1, i2), c = fold_right(ms, i2, n);
            const RMap ab_c = compose(compose(a, b), c), a_bc = compose(a, compose(b, c));
            for (int j = 0; j < 8; j++) {
                const i128 y = rnd_signed(rnd_int(1, 112));
                g_cases++;
                if (rapply(ab_c, y) != rapply(a_bc, y)) fail("associativity at y=" + str(y) + ": " + str(ab_c) + " against " + str(a_bc));
            }
            split = ab_c;
        }
        for (const RMap* m : {&l, &r, &t, (const RMap*)&split})
            if (!(m->t0 <= m->t1 && m->t1 <= m->t0 + ((i128)1 << (m->k + 1)))) fail("compose: result outside the family " + str(*m));
        const i128 centre = mode == 0 ? (i128)0 : rnd_signed(rnd_int(1, 112));
        for (int y = -300; y <= 300; y++) check_compose_at(ms, l, r, t, split, centre + y);
        for (int j = 0; j < 40; j++) check_compose_at(ms, l, r, t, split, rnd_signed(rnd_int(1, 112)));
        // around a step of the composed map
        const i128 edge = inv_min(l, rapply(l, centre));
        for (int y = -2; y <= 2; y++) check_compose_at(ms, l, r, t, split, edge + y);
    }
    if (!saw_down || !saw_up) fail("compose: the chains did not take both branches");
}

// ------------------------------------------------------------------------------------------------------------------------ 4.
static double make_double(u64 biased_exp, u64 mant) {
    const u64 bits = (biased_exp << 52) | (mant & 0xfffffffffffffull);
    double x;
    memcpy(&x, &bits, sizeof x);
    return x;
}
// x = mi 2^e by frexp / ldexp (a decomposition of its own: subnormals come out with fewer bits and a larger exponent)
static void decompose(double x, u64* mi, int* e) {
    int ex;
    const double m = frexp(x, &ex);
    *mi = (u64)ldexp(m, 53);
    *e = ex - 53;
}
static void check_to_grid_one(double x, int e0) {
    u64 mi; int e;
    decompose(x, &mi, &e);
    const int s = e - e0;
    i128 want; bool want_inexact;
    if (x == 0.0) { want = 0; want_inexact = false; }
    else if (s >= 0) { want = (i128)((u128)mi << s); want_inexact = false; }
    else if (s <= -64) { want = 0; want_inexact = true; }
    else { want = (i128)(mi >> -s); want_inexact = (mi & ((1ull << -s) - 1)) != 0; }
    bool inexact = false;
    const i128 got = to_grid(x, e0, &inexact);
    g_cases++;
    if (got != want || inexact != want_inexact)
        fail("to_grid: x=" + std::to_string(x) + " (mantissa " + std::to_string(mi) + " exponent " + std::to_string(e) + ") e0=" + std::to_string(e0) +
             ": " + str(got) + " inexact " + std::to_string((int)inexact) + ", brute force " + str(want) + " inexact " + std::to_string((int)want_inexact));
    if (!inexact) {                                  // on the grid: the round trip gives the same double back
        bool ok = true;
        const double back = from_grid(got, e0, &ok);
        u64 b0, b1;
        memcpy(&b0, &x, 8); memcpy(&b1, &back, 8);
        if (!ok || b0 != b1) fail("round trip: x=" + std::to_string(x) + " e0=" + std::to_string(e0) + " v=" + str(got) + " ok " + std::to_string((int)ok));
    }
}
static void check_grid() {
    // doubles of every kind; the grid placed so that sh = e - e0 (e: the exponent of the 53-bit mantissa, -1074 for subnormals)
    // takes every value from -70 to 69, the edges -64, -63, 0 and 69 with every double
    const int edges[] = {-64, -63, 0, 69, -65, -1, 1, -52, -53, 68};
    for (int it = 0; it < 60000; it++) {
        u64 be, mant;
        switch (it % 6) {
            case 0: be = 0; mant = rnd(); break;                                      // subnormal
            case 1: be = 0; mant = 1ull << rnd_int(0, 51); break;                     // subnormal, one bit
            case 2: be = (u64)rnd_int(1, 2046); mant = 0; break;                      // a power of two
            case 3: be = (u64)rnd_int(1, 2046); mant = rnd() << rnd_int(0, 52); break;  // trailing zeros
            case 4: be = (u64)rnd_int(1, 2046); mant = ~0ull; break;                  // all ones
            default: be = (u64)rnd_int(1, 2046); mant = rnd(); break;
        }
        const double x = make_double(be, mant);
        const int e = be ? (int)be - 1075 : -1074;
        for (int sh : edges) check_to_grid_one(x, e - sh);
        check_to_grid_one(x, e - rnd_int(-70, 69));
    }
    for (int e0 : {-1143, -1074, -1010, -100, 0, 40}) check_to_grid_one(0.0, e0);
    check_to_grid_one(make_double(0, 1), -1074);                                        // the smallest subnormal on its own grid
    check_to_grid_one(make_double(0, 1), -1074 - 69);
    check_to_grid_one(make_double(0, 1), -1073);
    // from_grid: values of up to 53 significant bits anywhere in 126 bits are doubles, anything longer is refused
    for (int it = 0; it < 60000; it++) {
        const int sig = rnd_int(1, 70), tz = rnd_int(0, 126 - sig);
        u128 u = (((u128)rnd() << 64) | rnd());
        if (sig < 128) u &= (((u128)1) << sig) - 1;
        u |= ((u128)1 << (sig - 1)) | 1;                                                // exactly `sig` significant bits
        const i128 v = (i128)(u << tz);
        const int e0 = rnd_int(-900, 800);
        bool ok = true;
        const double d = from_grid(v, e0, &ok);
        g_cases++;
        if (ok != (sig <= 53)) fail("from_grid: v=" + str(v) + " (" + std::to_string(sig) + " significant bits): ok " + std::to_string((int)ok));
        if (ok) {
            const double want = ldexp((double)(u64)u, tz + e0);                          // u < 2^53: exact
            bool inexact = false;
            const bool back = sig + tz - 53 < 70;                                        // (to_grid takes mantissas up to 69 bits above the grid)
            if (d != want || (back && (to_grid(d, e0, &inexact) != v || inexact))) fail("from_grid: v=" + str(v) + " e0=" + std::to_string(e0) + " gives " + std::to_string(d));
        }
    }
    bool ok = true;
    if (from_grid(0, -30, &ok) != 0.0 || !ok) fail("from_grid: zero");
    (void)from_grid(-1, -30, &ok);
    if (ok) fail("from_grid: a negative value passed");
    // level_of / bitlen against a loop
    for (int it = 0; it < 20000; it++) {
        const i128 v = rnd_signed(rnd_int(1, 126)) & (((i128)1 << 126) - 1);
        int bl = 0;
        for (u128 u = (u128)v; u; u >>= 1) bl++;
        g_cases++;
        if (bitlen(v) != bl || level_of(v) != (bl > 53 ? bl - 53 : 0)) fail("bitlen: v=" + str(v));
    }
}

int main() {
    check_rne();
    check_inv_min();
    check_compose();
    check_grid();
    printf("ok %lld\n", g_cases);
    return 0;
}
