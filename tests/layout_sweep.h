// The check the layout sweeps (geom_, meshsmooth_, meshdist_ and register_layout_sweep.cpp) make of one scratch layout of
// csrc/nfl_geom_layout.h.  The walk without a base (what nfl_*_bytes returns) and the walk over a buffer (what the entry
// point launches on) agree; every region starts 16-byte aligned, regions follow each other without overlap and the last one
// ends inside the buffer; one byte less is NFL_ESMALL and a misaligned or missing buffer NFL_EINVAL, in both orders of the
// two checks.  The buffer has exactly the size the first walk gave and the first and last byte of every region are written,
// so a region past the end is a heap overflow the sanitizer reports.  `what`, a, b, c name the layout in a failure's message.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "../nerf_fl_amd/csrc/nfl_geom_layout.h"

static long g_checked = 0;                                  // layouts that passed: the sweep prints "layouts ok <n>"

#define NG_CHECK(cond)                                                                  \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("layout invariant broken: %s (%s %lld %lld %lld)\n", #cond, what, a, b, c); \
            return false;                                                               \
        }                                                                               \
    } while (0)

template <int N>
static bool check(NgLayout<N> L, const char* what, long long a, long long b = 0, long long c = 0) {
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
