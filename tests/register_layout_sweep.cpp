// Host-side sweep of the scratch layout of the registration's moments (nr_moments_layout of csrc/nfl_geom_layout.h), built
// with -fsanitize=address,undefined by tests/test_register_layout_sanitizer_cpu.py: the checks tests/meshdist_layout_sweep.cpp
// makes of the mesh distance's.  For every size: the walk without a base and the walk over a buffer agree; the region starts
// 16-byte aligned and ends inside the buffer; one byte less is NFL_ESMALL and a misaligned or missing buffer NFL_EINVAL.  The
// buffer has exactly the size the first walk gave and the first and last byte of the region are written.  Prints
// "layouts ok <n>".
#include <cstdio>
#include <cstdlib>

#include "../nerf_fl_amd/csrc/nfl_geom_layout.h"

static long g_checked = 0;

#define NG_CHECK(cond)                                                                  \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("layout invariant broken: %s (%s %lld)\n", #cond, what, a);          \
            return false;                                                               \
        }                                                                               \
    } while (0)

template <int N>
static bool check(NgLayout<N> L, const char* what, long long a) {
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
