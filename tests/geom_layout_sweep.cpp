// Host-side sweep of the scratch layouts of the geometry entry points (csrc/nfl_geom_layout.h), built with
// -fsanitize=address,undefined by tests/test_geom_layout_sanitizer_cpu.py.  For every layout and size: the walk without a
// base (what nfl_*_bytes returns) and the walk over a buffer (what the entry point launches on) agree; every region
// starts 16-byte aligned, regions follow each other without overlap and the last one ends inside the buffer; one byte
// less is NFL_ESMALL and a misaligned buffer NFL_EINVAL.  The buffer has exactly the size the first walk gave and the
// first and last byte of every region are written, so a region past the end is a heap overflow the sanitizer reports.
// Prints "layouts ok <n>".
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../nerf_fl_amd/csrc/nfl_geom_layout.h"

static long g_checked = 0;

#define NG_CHECK(cond)                                                                  \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("layout invariant broken: %s (%s %lld %lld %lld)\n", #cond, what, a, b, c); \
            return false;                                                               \
        }                                                                               \
    } while (0)

template <int N>
static bool check(NgLayout<N> L, const char* what, long long a, long long b, long long c) {
    const size_t total = ng_bytes(L);
    NG_CHECK(total % 16 == 0);
    if (total == 0) {                                       // nothing to carve: every region is empty
        for (int i = 0; i < N; ++i) NG_CHECK(L.r[i].elem * L.r[i].count == 0);
        ++g_checked;
        return true;
    }
    char* buf = static_cast<char*>(aligned_alloc(16, total));
    NG_CHECK(buf != nullptr);
    NG_CHECK(ng_carve(L, buf, total - 1) == NFL_ESMALL && ng_carve(L, buf, 0, true) == NFL_ESMALL);
    NG_CHECK(ng_carve(L, buf + 4, total) == NFL_EINVAL && ng_carve(L, nullptr, total) == NFL_EINVAL);
    NG_CHECK(ng_carve(L, buf + 4, total - 1) == NFL_EINVAL && ng_carve(L, buf + 4, total - 1, true) == NFL_ESMALL);
    NG_CHECK(ng_carve(L, buf, total) == NFL_OK);
    const char* end = buf;                                  // where the region before ended
    for (int i = 0; i < N; ++i) {
        const size_t bytes = L.r[i].elem * L.r[i].count;
        NG_CHECK(L.at[i] >= end && (L.at[i] - buf) % 16 == 0 && L.at[i] - end < 16);
        NG_CHECK((size_t)(L.at[i] - buf) + bytes <= total);
        if (bytes) L.at[i][0] = L.at[i][bytes - 1] = (char)i;
        end = L.at[i] + bytes;
    }
    NG_CHECK((size_t)(end - buf) <= total && total - (size_t)(end - buf) < 16);   // the two walk modes end at the same place
    free(buf);
    ++g_checked;
    return true;
}

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
