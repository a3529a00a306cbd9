// Host-side sweep of the two scratch layouts of the mesh smoothing (na_layout, na_smooth_layout of csrc/nfl_geom_layout.h),
// built with -fsanitize=address,undefined by tests/test_meshsmooth_layout_sanitizer_cpu.py: the same checks
// tests/geom_layout_sweep.cpp makes of the older layouts.  For every size: the walk without a base and the walk over a
// buffer agree; every region starts 16-byte aligned, regions follow each other without overlap and the last one ends inside
// the buffer; one byte less is NFL_ESMALL and a misaligned buffer NFL_EINVAL.  The buffer has exactly the size the first
// walk gave and the first and last byte of every region are written.  Also the bounds emit puts on the totals.
// Prints "layouts ok <n>".
#include <cstdio>
#include <cstdlib>

#include "../nerf_fl_amd/csrc/nfl_geom_layout.h"

static long g_checked = 0;

#define NG_CHECK(cond)                                                                  \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("layout invariant broken: %s (%s %lld %lld)\n", #cond, what, a, b);  \
            return false;                                                               \
        }                                                                               \
    } while (0)

template <int N>
static bool check(NgLayout<N> L, const char* what, long long a, long long b) {
    const size_t total = ng_bytes(L);
    NG_CHECK(total % 16 == 0);
    if (total == 0) {
        for (int i = 0; i < N; ++i) NG_CHECK(L.r[i].elem * L.r[i].count == 0);
        ++g_checked;
        return true;
    }
    char* buf = static_cast<char*>(aligned_alloc(16, total));
    NG_CHECK(buf != nullptr);
    NG_CHECK(ng_carve(L, buf, total - 1) == NFL_ESMALL && ng_carve(L, buf + 4, total) == NFL_EINVAL);
    NG_CHECK(ng_carve(L, nullptr, total) == NFL_EINVAL && ng_carve(L, buf + 4, total - 1) == NFL_EINVAL);
    NG_CHECK(ng_carve(L, buf, total) == NFL_OK);
    const char* end = buf;
    for (int i = 0; i < N; ++i) {
        const size_t bytes = L.r[i].elem * L.r[i].count;
        NG_CHECK(L.at[i] >= end && (L.at[i] - buf) % 16 == 0 && L.at[i] - end < 16);
        NG_CHECK((size_t)(L.at[i] - buf) + bytes <= total);
        if (bytes) L.at[i][0] = L.at[i][bytes - 1] = (char)i;
        end = L.at[i] + bytes;
    }
    NG_CHECK((size_t)(end - buf) <= total && total - (size_t)(end - buf) < 16);
    free(buf);
    ++g_checked;
    return true;
}

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
