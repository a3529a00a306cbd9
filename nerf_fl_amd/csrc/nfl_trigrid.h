// nfl_trigrid.h -- what the queries against a mesh and its triangle grid share (nfl_meshdist.hip: the closest point;
// nfl_meshcast.hip: the cast and the occlusion; no other unit includes it): the view of a mesh with its grid, the host check
// of a grid's rows, the read of one row, and brute mode's staged tiles.  What a query DOES with a triangle -- nd_point_triangle
// against nc_test -- and how it walks the cells -- shells round a point against slabs along a ray -- stays with its unit, as a
// callable f(t, a, b, c) -> whether to stop: t the triangle's index, a, b, c its three corners (usable: in range and finite).
// The callables are lambdas marked NT_INLINE: they inline to the loops that stood in both units before.  DESIGN.md section 37.
#pragma once
#include "nfl_geom.h"

#define NT_TILE NM_THREADS                                  // triangles a workgroup stages in brute mode
#define NT_INLINE __attribute__((always_inline))            // on a lambda: what __forceinline__ is on a function

// a mesh and its grid as the kernels see them; off == nullptr: no rows (brute mode), and then E is 0
struct NtMesh {
    const float* ver;
    const int32_t* tri;
    i64 V, T;
    const i64* off;
    const int32_t* ent;
    i64 E;
    NdGrid G;
};

// the rows of a grid as an entry point is handed them.  What a call WITHOUT rows may pass for lo, cell and dims is the entry
// point's own rule
static inline bool nt_rows_ok(const int64_t* off, const int32_t* ent, int64_t E, const float* lo, float cell, const int32_t* dims) {
    if (!nd_grid_ok(lo, cell, dims) || ng_misaligned(off, 8)) return false;
    if (E < 0 || E > ND_MAX_ENTRIES) return false;
    return !(E && ng_bad(ent, 4));
}

// one row of the grid, read inside the arrays whatever it holds: f for every usable triangle the row lists, until f stops
template <typename F>
__device__ __forceinline__ void nt_row(const NtMesh& M, i64 cell, F&& f) {
    i64 r0 = M.off[cell], r1 = M.off[cell + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > M.E ? M.E : r1;
    for (i64 e = r0; e < r1; ++e) {
        const int32_t t = M.ent[e];
        if (t < 0 || t >= M.T) continue;
        float ca[3], cb[3], cc[3];
        if (!nm_corners(M.ver, M.tri, M.V, t, ca, cb, cc)) continue;
        if (f(t, ca, cb, cc)) return;
    }
}

// Brute mode: the workgroup stages NT_TILE triangles' corners in LDS (nine planes of floats and a flag, so the 64 lanes of a
// wave read ONE word each step: a broadcast), and a thread for which asks() holds tries the usable ones of the tile with f,
// whose result is not looked at: asks() is asked again at the next tile.  EVERY thread of the workgroup calls, whether it
// asks or not: it stages its triangle and reaches both barriers, the same trips for all.
template <typename Asks, typename F>
__device__ __forceinline__ void nt_tiles(const NtMesh& M, Asks&& asks, F&& f) {
    __shared__ float corner[9][NT_TILE];
    __shared__ int32_t usable[NT_TILE];
    for (i64 base = 0; base < M.T; base += NT_TILE) {
        const i64 t = base + threadIdx.x;
        float ca[3] = {0.f, 0.f, 0.f}, cb[3] = {0.f, 0.f, 0.f}, cc[3] = {0.f, 0.f, 0.f};
        const bool ok = t < M.T && nm_corners(M.ver, M.tri, M.V, t, ca, cb, cc);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            corner[k][threadIdx.x] = ca[k];
            corner[3 + k][threadIdx.x] = cb[k];
            corner[6 + k][threadIdx.x] = cc[k];
        }
        usable[threadIdx.x] = ok ? 1 : 0;
        __syncthreads();
        if (asks()) {
            const int len = (int)(M.T - base < NT_TILE ? M.T - base : NT_TILE);
            for (int j = 0; j < len; ++j) {
                if (!usable[j]) continue;
                const float ta[3] = {corner[0][j], corner[1][j], corner[2][j]};
                const float tb[3] = {corner[3][j], corner[4][j], corner[5][j]};
                const float tc[3] = {corner[6][j], corner[7][j], corner[8][j]};
                f((int32_t)(base + j), ta, tb, tc);
            }
        }
    }
}
