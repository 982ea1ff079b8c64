// Prints abc_weights_plan (abcsmc_amd/csrc/weights_plan.h), the plan behind the weight stage's two launchers, one line per case
// with every field by name, for tests/test_weights_dispatch.py to hold the tests' copy (tests/_weights_dispatch.py) against.
// Cases: P = 1..200 and 1024 x KDE mode x weight kernel x ABC_KDE_TOPN_MIN_PAIRS (its default, 0) x the (kn, K') below.
// g++ -O2 -std=c++17 tests/cxx/weights_plan_probe.cpp
#include <cstdio>
#include <initializer_list>

#include "../../abcsmc_amd/csrc/weights_plan.h"

int main() {
    static const size_t SHAPES[][2] = {
        {300, 700}, {150, 700}, {300, 1300}, {300, 2049}, {1, 700}, {255, 700}, {256, 700}, {257, 700},
        {40000, 100000}, {39999, 100000}, {100000, 100000}, {600000, 100000}, {256, 1000000}, {3084, 1000000}, {100000, 10000000},
        {300, 1}, {300, 31}, {300, 32}, {300, 33}, {300, 63}, {300, 64}, {300, 65}, {300, 127}, {300, 128}, {300, 129}};
    static const double MINP[] = {4.0e9, 0.0};
    for (size_t Pi = 1; Pi <= 201; Pi++) {
        const size_t P = Pi <= 200 ? Pi : 1024;
        for (int mode : {ABC_KDE_AUTO, ABC_KDE_FP64})
            for (int wk : {ABC_WEIGHT_GAUSSIAN, ABC_WEIGHT_EPANECHNIKOV})
                for (double minp : MINP)
                    for (const auto& sh : SHAPES) {
                        const abc_wplan pl = abc_weights_plan(P, sh[0], sh[1], mode, wk, minp);
                        printf("P=%zu kn=%zu Kp=%zu fp64=%d epan_in=%d minp=%.17g PP=%d NCH=%d epan=%d split=%d fold=%d topn=%d V=%d rb=%zu "
                               "slices=%zu nbt=%zu nat=%zu opa=%d opb=%d lim_i=%d\n",
                               P, sh[0], sh[1], mode == ABC_KDE_FP64, wk == ABC_WEIGHT_EPANECHNIKOV, minp, pl.PP, pl.NCH, (int)pl.epan,
                               (int)pl.split, (int)pl.fold, (int)pl.topn, pl.V, pl.rb, pl.slices, pl.nbt, pl.nat, pl.opa, pl.opb, pl.lim_i);
                    }
    }
    return 0;
}
