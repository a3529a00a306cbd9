// Host-side sweep of the scratch layouts of the geometry entry points (csrc/nfl_geom_layout.h), built with
// -fsanitize=address,undefined by tests/test_geom_layout_sanitizer_cpu.py.  Every layout and size goes through the check of
// tests/layout_sweep.h, which says what it asserts.  Also what the entry points refuse before they look at a layout.
// Prints "layouts ok <n>".
#include <initializer_list>

#include "layout_sweep.h"

int main() {
    const long long mesh[] = {0, 1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 5000, 100003};
    const long long big = 2048ll * 2048 + 1;                // the first size with three scan levels
    bool ok = true;
    for (long long V : mesh)
        for (long long T : mesh) {
            ok = ok && nm_sizes_ok(V, T);
            ok = ok && check(nm_label_layout(V), "label", V, T, 0);
            ok = ok && check(nm_compact_layout(V, T), "compact", V, T, 0);
            ok = ok && check(nc_layout(V, T), "simplify", V, T, 0);
        }
    ok = ok && check(nm_label_layout(big), "label", big, 0, 0);
    ok = ok && check(nm_compact_layout(big, 1), "compact", big, 1, 0) && check(nm_compact_layout(1, big), "compact", 1, big, 0);
    ok = ok && check(nc_layout(1, big), "simplify", 1, big, 0);
    const int dims[] = {2, 3, 31, 32, 33, 64, 65, 255, 256, 257};
    for (int nx : dims)
        for (int ny : {2, 3, 7})
            for (int nz : {2, 5}) {
                ok = ok && ng_dims_ok(nx, ny, nz);
                ok = ok && check(ns_layout(nx, ny, nz), "surface", nx, ny, nz);
                ok = ok && check(no_layout(nx, ny, nz), "occupancy", nx, ny, nz);
            }
    ok = ok && check(ns_layout(1025, 2, 2), "surface", 1025, 2, 2) && check(no_layout(1025, 2, 2), "occupancy", 1025, 2, 2);
    // what the entry points refuse before they look at a layout
    ok = ok && !nm_sizes_ok(-1, 0) && !nm_sizes_ok(0, -1) && !nm_sizes_ok(1ll << 31, 0) && !nm_sizes_ok(0, INT32_MAX / 3 + 1);
    ok = ok && !ng_dims_ok(1, 2, 2) && !ng_dims_ok(2, 65536, 2) && !ng_dims_ok(2, 2, 65536) && !ng_dims_ok(1025, 1024, 1024);
    if (!ok) return 1;
    printf("layouts ok %ld\n", g_checked);
    return 0;
}
