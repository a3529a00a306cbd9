// Host-side sweep of the scratch layout of the registration's moments (nr_moments_layout of csrc/nfl_geom_layout.h), built
// with -fsanitize=address,undefined by tests/test_register_layout_sanitizer_cpu.py.  Every size goes through the check of
// tests/layout_sweep.h, which says what it asserts.  Also the row's columns.  Prints "layouts ok <n>".
#include "layout_sweep.h"

int main() {
    const long long sizes[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000, 70001, 100003};
    bool ok = true;
    for (long long n : sizes) ok = ok && check(nr_moments_layout(n), "moments", n);
    ok = ok && check(nr_moments_layout(1024 * 256 + 1), "moments", 1024 * 256 + 1);
    ok = ok && check(nr_moments_layout(INT32_MAX), "moments", INT32_MAX);
    // a row of NFL_REGISTER_COLUMNS doubles per workgroup of the reduction: one per 256 pairs, 1024 at the most
    ok = ok && NFL_REGISTER_COLUMNS == 55 && nr_moments_layout(70001).r[NR_M_PARTS].elem == 8 * NFL_REGISTER_COLUMNS;
    ok = ok && nr_moments_layout(0).r[NR_M_PARTS].count == 0 && nr_moments_layout(256).r[NR_M_PARTS].count == 1;
    ok = ok && nr_moments_layout(257).r[NR_M_PARTS].count == 2 && nr_moments_layout(70001).r[NR_M_PARTS].count == 274;
    ok = ok && nr_moments_layout(INT32_MAX).r[NR_M_PARTS].count == 1024 && ng_bytes(nr_moments_layout(INT32_MAX)) == 1024 * 440;
    // the row's runs lie one after the other and fill it
    ok = ok && NFL_REGISTER_SUM_P == 2 && NFL_REGISTER_SUM_Q == NFL_REGISTER_SUM_P + 3 && NFL_REGISTER_SUM_PP == NFL_REGISTER_SUM_Q + 3;
    ok = ok && NFL_REGISTER_SUM_QQ == NFL_REGISTER_SUM_PP + 1 && NFL_REGISTER_SUM_PQ == NFL_REGISTER_SUM_QQ + 1;
    ok = ok && NFL_REGISTER_ATA == NFL_REGISTER_SUM_PQ + 9 && NFL_REGISTER_ATB == NFL_REGISTER_ATA + 28;
    ok = ok && NFL_REGISTER_SUM_RR == NFL_REGISTER_ATB + 7 && NFL_REGISTER_COLUMNS == NFL_REGISTER_SUM_RR + 1;
    if (!ok) return 1;
    printf("layouts ok %ld\n", g_checked);
    return 0;
}
