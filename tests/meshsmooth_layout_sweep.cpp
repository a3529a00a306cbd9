// Host-side sweep of the two scratch layouts of the mesh smoothing (na_layout, na_smooth_layout of csrc/nfl_geom_layout.h),
// built with -fsanitize=address,undefined by tests/test_meshsmooth_layout_sanitizer_cpu.py.  Every size goes through the
// check of tests/layout_sweep.h, which says what it asserts.  Also the bounds emit puts on the totals.
// Prints "layouts ok <n>".
#include "layout_sweep.h"

int main() {
    const long long mesh[] = {0, 1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 5000, 100003};
    const long long big = 2048ll * 2048 + 1;                // the first size with three scan levels
    bool ok = true;
    for (long long V : mesh) {
        ok = ok && check(na_smooth_layout(V), "smooth", V, 0);
        for (long long T : mesh) ok = ok && check(na_layout(V, T), "adjacency", V, T);
    }
    ok = ok && check(na_layout(big, 1), "adjacency", big, 1) && check(na_layout(1, big), "adjacency", 1, big);
    ok = ok && check(na_smooth_layout(big), "smooth", big, 0);
    // the sizes of the largest mesh the calls take do not wrap
    const NgLayout<NA_REGIONS> L = na_layout(INT32_MAX, INT32_MAX / 3);
    ok = ok && L.r[NA_CAND].count == 6ull * (INT32_MAX / 3) && ng_bytes(L) > 48ull * (INT32_MAX / 3) + 29ull * INT32_MAX;
    // the totals emit takes
    ok = ok && na_totals_ok(4, 12, 24) && na_totals_ok(4, 0, 0) && na_totals_ok(0, 0, 0) && na_totals_ok(INT32_MAX / 3, INT32_MAX / 3 * 3ll, 0);
    ok = ok && !na_totals_ok(4, 13, 0) && !na_totals_ok(4, 12, 25) && !na_totals_ok(4, -1, 0) && !na_totals_ok(4, 0, -1) && !na_totals_ok(4, 0, 1);
    if (!ok) return 1;
    printf("layouts ok %ld\n", g_checked);
    return 0;
}
