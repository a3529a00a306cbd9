// Host-side sweep of the three scratch layouts of the mesh edges (ne_layout, nl_layout, nf_layout of csrc/nfl_geom_layout.h),
// built with -fsanitize=address,undefined by tests/test_meshedge_layout_sanitizer_cpu.py.  Every size goes through the check
// of tests/layout_sweep.h, which says what it asserts.  Also the bounds the emit calls put on the totals, and the rounds of
// the pointer doubling.  Prints "layouts ok <n>".
#include "layout_sweep.h"

int main() {
    // 0 and 1, the wave, the scan's tile (2048) over 3 T half-edges (T = 682, 683) and over T, two scan levels
    const long long mesh[] = {0, 1, 2, 63, 64, 65, 682, 683, 2047, 2048, 2049, 100003};
    const long long big = 2048ll * 2048 + 1;                // the first size with three scan levels
    bool ok = true;
    for (long long V : mesh) {
        ok = ok && check(nl_layout(V), "loops", V) && check(nf_layout(V), "fill", V);
        for (long long T : mesh) ok = ok && check(ne_layout(V, T), "edges", V, T);
    }
    ok = ok && check(ne_layout(big, 1), "edges", big, 1) && check(ne_layout(1, big), "edges", 1, big);
    ok = ok && check(nl_layout(big), "loops", big) && check(nf_layout(big), "fill", big);
    // the sizes of the largest mesh the calls take do not wrap
    const long long TMAX = INT32_MAX / 3;
    const NgLayout<NE_REGIONS> E = ne_layout(INT32_MAX, TMAX);
    ok = ok && E.r[NE_HOFF].count == 3ull * TMAX && ng_bytes(E) > 87ull * TMAX + 12ull * INT32_MAX;
    const NgLayout<NL_REGIONS> L = nl_layout(TMAX);
    ok = ok && L.r[NL_RANK].count == 3ull * TMAX && L.r[NL_CEN].count == (size_t)TMAX && ng_bytes(L) > 148ull * TMAX;
    ok = ok && ng_bytes(nf_layout(TMAX)) > 28ull * TMAX && nm_sizes_ok(INT32_MAX, TMAX) && !nm_sizes_ok(0, TMAX + 1);
    // the totals the emit calls take
    ok = ok && ne_totals_ok(4, 12, 12) && ne_totals_ok(4, 0, 0) && ne_totals_ok(0, 0, 0) && ne_totals_ok(TMAX, 3 * TMAX, 3 * TMAX);
    ok = ok && !ne_totals_ok(4, 13, 0) && !ne_totals_ok(4, 0, 13) && !ne_totals_ok(4, -1, 0) && !ne_totals_ok(4, 0, -1);
    ok = ok && nl_totals_ok(4, 4, 12) && nl_totals_ok(4, 0, 0) && !nl_totals_ok(4, 5, 0) && !nl_totals_ok(4, 0, 13);
    ok = ok && !nl_totals_ok(4, -1, 0) && !nl_totals_ok(4, 0, -1) && nl_totals_ok(TMAX, TMAX, 3 * TMAX);
    ok = ok && nf_totals_ok(2, 6, 2, 6) && nf_totals_ok(2, 6, 0, 0) && !nf_totals_ok(2, 6, 3, 0) && !nf_totals_ok(2, 6, 0, 7);
    ok = ok && !nf_totals_ok(2, 6, -1, 0) && !nf_totals_ok(2, 6, 0, -1);
    // ceil(log2 B) + 1 rounds: the pointer reaches 2^rounds ahead, at least around a cycle of B
    const long long bs[] = {0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 3 * TMAX};
    const int want[] = {1, 1, 2, 3, 3, 4, 11, 11, 12, 32};
    for (int k = 0; k < 10; ++k) ok = ok && nl_rounds(bs[k]) == want[k] && (1ll << (nl_rounds(bs[k]) - 1)) >= bs[k];
    if (!ok) return 1;
    printf("layouts ok %ld\n", g_checked);
    return 0;
}
