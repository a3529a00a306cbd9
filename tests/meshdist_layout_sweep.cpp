// Host-side sweep of the three scratch layouts of the mesh distance (nd_grid_layout, nd_sample_layout, nd_reduce_layout of
// csrc/nfl_geom_layout.h), built with -fsanitize=address,undefined by tests/test_meshdist_layout_sanitizer_cpu.py.  Every
// size goes through the check of tests/layout_sweep.h, which says what it asserts.  Also the reduction's workgroups and the
// limits the grid puts on its sizes.  Prints "layouts ok <n>".
#include "layout_sweep.h"

int main() {
    const long long sizes[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000, 70001, 100003};
    const long long big = 2048ll * 2048 + 1;                // the first size with three scan levels
    bool ok = true;
    for (long long n : sizes) {
        if (n) ok = ok && check(nd_grid_layout(n), "grid", n);          // a grid has a cell
        ok = ok && check(nd_sample_layout(n), "sample", n) && check(nd_reduce_layout(n), "reduce", n);
    }
    ok = ok && check(nd_grid_layout(big), "grid", big) && check(nd_sample_layout(big), "sample", big);
    ok = ok && check(nd_reduce_layout(big), "reduce", big) && check(nd_reduce_layout(INT32_MAX), "reduce", INT32_MAX);
    // the reduction's workgroups: one per 256 elements, 1024 at the most, and a row of 13 doubles each
    ok = ok && nd_reduce_blocks(0) == 0 && nd_reduce_blocks(1) == 1 && nd_reduce_blocks(256) == 1 && nd_reduce_blocks(257) == 2;
    ok = ok && nd_reduce_blocks(70001) == 274 && nd_reduce_blocks(1024 * 256 + 1) == 1024 && nd_reduce_blocks(INT32_MAX) == 1024;
    ok = ok && nd_reduce_layout(70001).r[ND_R_PARTS].elem == 8 * NFL_MESHDIST_COLUMNS && NFL_MESHDIST_COLUMNS == 13;
    // the sizes of the largest grid and mesh the calls take do not wrap
    ok = ok && ng_bytes(nd_grid_layout(NG_MAX_POINTS)) > 12ull * NG_MAX_POINTS;
    ok = ok && ng_bytes(nd_sample_layout(INT32_MAX / 3)) > 12ull * (INT32_MAX / 3);
    // the grid's limits
    const int32_t good[3] = {1, 65535, 4}, zero[3] = {4, 0, 4}, wide[3] = {65536, 1, 1}, many[3] = {1024, 1024, 1025}, most[3] = {1024, 1024, 1024};
    ok = ok && nd_dims_ok(good) && nd_dims_ok(most) && !nd_dims_ok(zero) && !nd_dims_ok(wide) && !nd_dims_ok(many);
    if (!ok) return 1;
    printf("layouts ok %ld\n", g_checked);
    return 0;
}
