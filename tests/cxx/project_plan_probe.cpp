// Prints abc_project_plan (abcsmc_amd/csrc/project_plan.h), the plan behind the projection's three launchers, one line per case,
// for tests/test_project_dispatch.py to hold the tests' copy (tests/_project_dispatch.py) against.  A line is the mode's letter
// (D distance, S scores only, F fused), the request, "->", the plan:
//   D M A n ldx x_aligned dist_aligned            -> main KC rows tail tail_rows pad lds lds_main grid tail_grid
//   S M A n ldx x_aligned s_aligned               -> declined main KC rows lds lds_main grid
//   F M A n ldx x_aligned dist_aligned s_aligned row_test sld -> declined main KC rows lds lds_main grid
// Cases: M and n on both sides of every threshold x A = 0..97 (A = 0: the simple filter in distance mode) x both parities of the
// leading dimension x every alignment; fused: row_test in {0, 1, n / 2, n} x both parities of sld.
// g++ -O2 -std=c++17 tests/cxx/project_plan_probe.cpp
#include <cstdio>

#include "../../abcsmc_amd/csrc/project_plan.h"

static const char* name(abc_pj_kernel k) {
    switch (k) {
        case PJ_SIMPLE: return "simple";
        case PJ_WIDE: return "wide";
        case PJ_MFMA: return "mfma";
        case PJ_DIST2_LDS: return "dist2_lds";
        case PJ_DIST2: return "dist2";
        case PJ_DIST: return "dist";
        default: return "none";
    }
}

int main() {
    static const size_t MS[] = {1, 2, 20, 248, 249, 252, 511, 512, 560, 561, 1023, 1024, 1100};
    static const size_t NS[] = {0, 1, 2, 3, 1000, 1001, 524288, 524290, 1048576, 1048577, 2097152, 2097154};
    static char buf[1 << 20];
    setvbuf(stdout, buf, _IOFBF, sizeof(buf));
    for (size_t M : MS)
        for (size_t A = 0; A <= 97; A++)
            for (size_t n : NS)
                for (size_t ldx = n + 2; ldx <= n + 3; ldx++) {
                    for (int al = 0; al < 4; al++) {        // (the second pointer: dist in distance mode, S in scores mode)
                        const bool xa = al & 1, pa = al & 2;
                        const abc_pj_plan d = abc_project_plan({PJ_DISTANCE, n, ldx, M, A, A == 0, 0, 0, xa, pa, true});
                        printf("D %zu %zu %zu %zu %d %d -> %s %d %zu %s %zu %d %zu %zu %u %u\n", M, A, n, ldx, xa, pa, name(d.main), d.KC,
                               d.rows, name(d.tail), d.tail_rows, (int)d.pad, d.lds, d.lds_main, d.grid, d.tail_grid);
                        const abc_pj_plan s = abc_project_plan({PJ_SCORES, n, ldx, M, A, false, 0, n, xa, true, pa});
                        printf("S %zu %zu %zu %zu %d %d -> %d %s %d %zu %zu %zu %u\n", M, A, n, ldx, xa, pa, (int)s.declined, name(s.main),
                               s.KC, s.rows, s.lds, s.lds_main, s.grid);
                    }
                    const size_t RT[4] = {0, 1, n / 2, n};
                    for (int al = 0; al < 8; al++)
                        for (int r = 0; r < 4; r++)
                            for (size_t sld = n + 4; sld <= n + 5; sld++) {
                                const bool xa = al & 1, da = al & 2, sa = al & 4;
                                const abc_pj_plan f = abc_project_plan({PJ_FUSED, n, ldx, M, A, false, RT[r], sld, xa, da, sa});
                                printf("F %zu %zu %zu %zu %d %d %d %zu %zu -> %d %s %d %zu %zu %zu %u\n", M, A, n, ldx, xa, da, sa, RT[r], sld,
                                       (int)f.declined, name(f.main), f.KC, f.rows, f.lds, f.lds_main, f.grid);
                            }
                }
    return 0;
}
