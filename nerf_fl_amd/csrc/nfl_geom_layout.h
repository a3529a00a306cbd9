// nfl_geom_layout.h -- the host arithmetic of the geometry entry points.  The scratch of every one of them (surface, mesh,
// occupancy, simplify, smoothing, mesh distance, registration, mesh edges) is written ONCE, as an ordered list of regions, and one
// routine walks it.  Without a base the walk gives the size (what the nfl_*_bytes functions return); with the caller's
// buffer it gives the pointers (what the entry points launch on), so the two cannot disagree.  Beside the layouts: the size
// limits, and the pointer and finite checks every entry point makes of its arguments (ng_misaligned, ng_bad, ng_finite).
// Plain C++ with no HIP in it: the tests/*_layout_sweep.cpp programs build it with g++ under the sanitizers.  DESIGN.md
// sections 22 and 35.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nerf_fl_amd.h"

typedef int64_t i64;

#define NG_MAX_POINTS (1ll << 30)
#define NG_MAX_DIM 65535                                    // rows and planes of a lattice are grid dimensions
#define NS_TILE 256                                         // points of an x-row in one slab of the surface kernels
#define NM_SCAN_THREADS 512
#define NM_SCAN_ITEMS 4
#define NM_SCAN_TILE (NM_SCAN_THREADS * NM_SCAN_ITEMS)      // 2048: 2^31 elements -> 2^20 -> 2^9 -> 1 tile sums
#define NM_SCAN_LEVELS 3

static inline size_t ng_pad(size_t bytes) { return (bytes + 15) / 16 * 16; }
static inline i64 ng_cdiv(i64 a, i64 b) { return (a + b - 1) / b; }
static inline size_t ng_max(size_t a, size_t b) { return a > b ? a : b; }

// The pointer checks of every geometry entry point; the only uintptr_t casts of the geometry sources are these.  A null
// pointer is aligned: an optional argument is checked with ng_misaligned alone, a required one with ng_bad.
static inline bool ng_misaligned(const void* p, int align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }
static inline bool ng_bad(const void* p, int align) { return !p || ng_misaligned(p, align); }      // absent or misaligned
// neither an infinity nor a NaN (host arguments; the kernels' is ng_is_finite of nfl_geom.h)
static inline bool ng_finite(float x) { return x - x == 0.f; }
static inline bool ng_finite(double x) { return x - x == 0.0; }

// a lattice the surface and occupancy kernels take
static inline bool ng_dims_ok(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2 || ny > NG_MAX_DIM || nz > NG_MAX_DIM) return false;
    return (long long)nx * ny <= NG_MAX_POINTS && (long long)nx * ny * nz <= NG_MAX_POINTS;
}
// a mesh the mesh and simplify kernels take: int32 indices
static inline bool nm_sizes_ok(i64 V, i64 T) { return V >= 0 && T >= 0 && V <= INT32_MAX && T <= INT32_MAX / 3; }
// the mesh of a mesh distance or registration call: sizes, the pointers a non-zero size needs, and BOTH pointers aligned
// even where the mesh is empty (nmc_mesh_ok of nfl_meshray.h does not look at the pointer of an empty side)
static inline bool nd_mesh_ok(const float* ver, const int32_t* tri, i64 V, i64 T) {
    if (!nm_sizes_ok(V, T) || (V && !ver) || (T && !tri)) return false;
    return !ng_misaligned(ver, 4) && !ng_misaligned(tri, 4);
}

// what nm_scan (nfl_mesh_scan.hip) needs for n elements: the tile sums of all levels above the elements, 8 B each
static inline size_t nm_scan_bytes(i64 n) {
    size_t entries = 0;
    for (i64 m = ng_cdiv(n, NM_SCAN_TILE); m > 1; m = ng_cdiv(m, NM_SCAN_TILE)) entries += (size_t)m;
    return ng_pad(entries * 8);
}
// slots of a simplify hash table: the power of two >= 2 n (at least 2); 0 for n == 0
static inline uint64_t nc_cap(i64 n) {
    if (n <= 0) return 0;
    uint64_t c = 2;
    while (c < 2 * (uint64_t)n) c <<= 1;
    return c;
}
static inline int ns_ntx(int nx) { return (nx + NS_TILE - 1) / NS_TILE; }      // slabs per x-row
static inline int no_words(int n) { return (n + 31) / 32; }

struct NgRegion { size_t elem, count; };                    // bytes per element, elements

// N regions in the order they lie in the scratch, each padded to 16 B
template <int N>
struct NgLayout {
    NgRegion r[N];
    char* at[N];            // where region i starts: set by ng_carve
    template <typename T>
    T* get(int i) const { return reinterpret_cast<T*>(at[i]); }
};

// The one walk.  Returns the offset at which the last region ends; with a base also at[i] = the start of region i.
static inline size_t ng_walk(const NgRegion* r, int n, void* base, char** at) {
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (base) at[i] = static_cast<char*>(base) + off;
        off += ng_pad(r[i].elem * r[i].count);
    }
    return off;
}

template <int N>
static inline size_t ng_bytes(const NgLayout<N>& L) { return ng_walk(L.r, N, nullptr, nullptr); }

// The check every entry point makes of the caller's scratch, then the carve.  A buffer that is both misaligned and too
// small is NFL_EINVAL, except for the surface calls (`size_first`), which have always looked at the size first.
template <int N>
static inline int ng_carve(NgLayout<N>& L, void* scratch, size_t scratch_bytes, bool size_first = false) {
    if (!scratch) return NFL_EINVAL;
    const bool misaligned = ng_misaligned(scratch, 8), small = scratch_bytes < ng_bytes(L);
    if (small && (size_first || !misaligned)) return NFL_ESMALL;
    if (misaligned) return NFL_EINVAL;
    ng_walk(L.r, N, scratch, L.at);
    return NFL_OK;
}

// ---- surface: nfl_surface_count / nfl_surface_emit
enum { NS_REC, NS_SUMS, NS_REGIONS };
static inline NgLayout<NS_REGIONS> ns_layout(int nx, int ny, int nz) {
    return {{{4, (size_t)nx * ny * nz},                     // uint32 per point: mask << 16 | vertex offset inside the slab
             {16, (size_t)ns_ntx(nx) * ny * nz}}, {}};      // (vertices, triangles) int64 per slab, then their prefix sums
}

// ---- occupancy: nfl_occ_build
enum { NO_P, NO_X, NO_REGIONS };
static inline NgLayout<NO_REGIONS> no_layout(int nx, int ny, int nz) {
    return {{{4, (size_t)nz * ny * no_words(nx)},           // (nz, ny, wpx) point flags; after the y pass (nz, cy, wx)
             {4, (size_t)nz * ny * no_words(nx - 1)}}, {}}; // (nz, ny, wx)
}

// ---- mesh: nfl_mesh_label
enum { NM_L_PARENT, NM_L_FLAG, NM_L_RANK, NM_L_SUMS, NM_L_REGIONS };
static inline NgLayout<NM_L_REGIONS> nm_label_layout(i64 V) {
    const size_t v = (size_t)V;
    return {{{4, v},                                        // int32 parent of the union-find
             {4, v},                                        // int32 1 = root
             {8, v},                                        // int64 roots before v
             {1, nm_scan_bytes(V)}}, {}};                   // tile sums of the scan
}

// ---- mesh: nfl_mesh_compact_count / nfl_mesh_compact_emit.  ONE region of tile sums, sized for the longer of the two
// scans: the vertex scan has finished with it (its sums are added back) before the triangle scan, next in the stream, starts.
enum { NM_C_FLAG_V, NM_C_OFF_V, NM_C_FLAG_T, NM_C_OFF_T, NM_C_SUMS, NM_C_REGIONS };
static inline NgLayout<NM_C_REGIONS> nm_compact_layout(i64 V, i64 T) {
    const size_t v = (size_t)V, t = (size_t)T;
    return {{{4, v},                                        // int32 1 = kept
             {8, v},                                        // int64 kept vertices before v
             {4, t},
             {8, t},
             {1, ng_max(nm_scan_bytes(V), nm_scan_bytes(T))}}, {}};
}

// ---- simplify: nfl_mesh_simplify_count / nfl_mesh_simplify_emit
enum { NC_VKEY, NC_VMIN, NC_VSLOT, NC_FLAG_V, NC_RANK, NC_CANON, NC_TOWNER, NC_TMIN, NC_TSLOT, NC_FLAG_T, NC_OFF_T, NC_SUMS,
       NC_COUNT, NC_FIXED, NC_QUADRIC, NC_REGIONS };
static inline NgLayout<NC_REGIONS> nc_layout(i64 V, i64 T) {
    const size_t v = (size_t)V, t = (size_t)T, cv = (size_t)nc_cap(V), ct = (size_t)nc_cap(T);
    return {{{8, cv},                                       // uint64 keys, NC_EMPTY_KEY when free
             {4, cv},                                       // int32 smallest vertex index of the slot
             {4, v},                                        // uint32 slot of the vertex
             {4, v},                                        // int32 1 = leader of its cluster
             {8, v},                                        // int64 leaders before v
             {12, t},                                       // int32 x 3 new ids, smallest first; [0] = -1: dropped
             {4, ct},                                       // int32 the triangle that claimed the slot, -1 when free
             {4, ct},                                       // int32 smallest triangle index of the slot
             {4, t},                                        // uint32 slot of the triangle, NC_NO_SLOT when dropped
             {4, t},                                        // int32 1 = survivor
             {8, t},                                        // int64 survivors before t
             {1, ng_max(nm_scan_bytes(V), nm_scan_bytes(T))},       // tile sums of the longer of the two scans
             {4, v},                                        // int32 members of cluster c -- emit; the first V' are used
             {72, v},                                       // int64 x 9 position, normal, colour sums
             {72, v}}, {}};                                 // double x 9 A (xx xy xz yy yz zz), b
}

// ---- mesh smoothing: nfl_mesh_adjacency_count / nfl_mesh_adjacency_emit
enum { NA_CNT, NA_CUR, NA_DEG, NA_TOFF, NA_OFF, NA_INC, NA_CAND, NA_TMP, NA_FLAG, NA_SUMS, NA_REGIONS };
static inline NgLayout<NA_REGIONS> na_layout(i64 V, i64 T) {
    const size_t v = (size_t)V, t = (size_t)T;
    return {{{4, v},                                        // int32 incident entries of v
             {4, v},                                        // int32 cursor of v while its row is filled
             {4, v},                                        // int32 length of the neighbour row of v
             {8, v},                                        // int64 incident entries before v
             {8, v},                                        // int64 neighbours before v
             {4, 3 * t},                                    // int32 incident entries 3 t + c, the row of v at its offset
             {4, 6 * t},                                    // int32 neighbour rows, the row of v at twice its incident offset
             {4, 6 * t},                                    // int32 where a long row is sorted from
             {1, v},                                        // uint8 boundary flag
             {1, nm_scan_bytes(V)}}, {}};                   // tile sums of the two scans, one after the other
}
// the bounds of the totals emit takes: I <= 3 T, N <= 2 I
static inline bool na_totals_ok(i64 T, i64 I, i64 N) { return I >= 0 && N >= 0 && I <= 3 * T && N <= 2 * I; }

// ---- mesh smoothing: nfl_mesh_smooth
enum { NA_S_PING, NA_S_REGIONS };
static inline NgLayout<NA_S_REGIONS> na_smooth_layout(i64 V) {
    return {{{12, (size_t)V}}, {}};                         // fp32 x 3 the positions of every other step
}

// ---- mesh distance: nfl_trigrid_count / nfl_trigrid_emit
#define ND_MAX_ENTRIES ((i64)INT32_MAX)                    // entries of a grid's rows, samples of a surface, distances of a run
#define ND_MAX_SAMPLES_PER_TRIANGLE 16777216.0f             // 2^24
#define ND_REDUCE_MAX_BLOCKS 1024
static inline bool nd_dims_ok(const int32_t* dims) {
    for (int k = 0; k < 3; ++k)
        if (dims[k] < 1 || dims[k] > NG_MAX_DIM) return false;
    return (i64)dims[0] * dims[1] * dims[2] <= NG_MAX_POINTS;
}
enum { ND_G_CNT, ND_G_OFF, ND_G_SUMS, ND_G_REGIONS };
static inline NgLayout<ND_G_REGIONS> nd_grid_layout(i64 cells) {
    const size_t c = (size_t)cells;
    return {{{4, c},                                        // int32 triangles listed in cell c; the cursor of c while emit fills
             {8, c},                                        // int64 entries before cell c
             {1, nm_scan_bytes(cells)}}, {}};               // tile sums of the scan
}

// ---- mesh distance: nfl_mesh_sample_count / nfl_mesh_sample_emit
enum { ND_S_CNT, ND_S_OFF, ND_S_SUMS, ND_S_REGIONS };
static inline NgLayout<ND_S_REGIONS> nd_sample_layout(i64 T) {
    const size_t t = (size_t)T;
    return {{{4, t},                                        // int32 samples of triangle t
             {8, t},                                        // int64 samples before triangle t
             {1, nm_scan_bytes(T)}}, {}};
}

// ---- mesh distance: nfl_meshdist_reduce
static inline i64 nd_reduce_blocks(i64 n) {
    const i64 g = ng_cdiv(n, 256);
    return g < ND_REDUCE_MAX_BLOCKS ? g : ND_REDUCE_MAX_BLOCKS;
}
enum { ND_R_PARTS, ND_R_REGIONS };
static inline NgLayout<ND_R_REGIONS> nd_reduce_layout(i64 n) {
    return {{{8 * NFL_MESHDIST_COLUMNS, (size_t)nd_reduce_blocks(n)}}, {}};    // one fp64 row per workgroup
}

// ---- registration: nfl_register_moments.  The workgroups are the reduction's: nd_reduce_blocks
enum { NR_M_PARTS, NR_M_REGIONS };
static inline NgLayout<NR_M_REGIONS> nr_moments_layout(i64 n) {
    return {{{8 * NFL_REGISTER_COLUMNS, (size_t)nd_reduce_blocks(n)}}, {}};    // one fp64 row per workgroup
}

// ---- mesh edges: nfl_mesh_edges_count / nfl_mesh_edges_emit.  Per-edge regions are 3 T long: every edge has a half-edge
enum { NE_OWN, NE_EOFF, NE_HE, NE_CNT, NE_CUR, NE_HOFF, NE_TMP, NE_EH, NE_KIND, NE_SUMS, NE_RAW, NE_REGIONS };
static inline NgLayout<NE_REGIONS> ne_layout(i64 V, i64 T) {
    const size_t v = (size_t)V, h = 3 * (size_t)T;
    return {{{4, v},                                        // int32 edges vertex a owns: its neighbours b > a
             {8, v},                                        // int64 edges before those of a
             {4, h},                                        // int32 edge of half-edge h, -1: none
             {4, h},                                        // int32 half-edges on edge e
             {4, h},                                        // int32 cursor of e while its row is filled
             {8, h},                                        // int64 half-edges before the row of e
             {4, h},                                        // int32 the rows in order of arrival
             {4, h},                                        // int32 the rows ascending
             {1, h},                                        // uint8 kind of e
             {1, ng_max(nm_scan_bytes(V), nm_scan_bytes(3 * T))},   // tile sums of the two scans, one after the other
             {8, 2}}, {}};                                  // int64 E and H as the scans gave them
}
// the bounds of the totals emit takes: every edge has a half-edge, every half-edge lies on one edge at most
static inline bool ne_totals_ok(i64 T, i64 E, i64 H) { return E >= 0 && H >= 0 && E <= 3 * T && H <= 3 * T; }

// ---- mesh edges: nfl_mesh_loops_count / nfl_mesh_loops_emit.  A loop has at least 3 half-edges: per-loop regions are T long
enum { NL_SUCC, NL_PTR0, NL_MIN0, NL_PTR1, NL_MIN1, NL_ROOT, NL_FLAG, NL_RANK, NL_POS, NL_LEN, NL_LOFF, NL_PER, NL_CEN, NL_SUMS,
       NL_RAW, NL_REGIONS };
static inline NgLayout<NL_REGIONS> nl_layout(i64 T) {
    const size_t t = (size_t)T, h = 3 * t;
    return {{{4, h},                                        // int32 successor; -1: a dead end; -2: not a boundary half-edge
             {4, h}, {4, h},                                // int32 the pointer and the smallest half-edge ahead, even rounds
             {4, h}, {4, h},                                // the same, odd rounds
             {4, h},                                        // int32 the loop's smallest half-edge, -1: on no loop
             {4, h},                                        // int32 1 = the smallest of its loop
             {8, h},                                        // int64 loops before that of h
             {4, h},                                        // int32 place of h in its loop
             {4, t},                                        // int32 length of loop l
             {8, t},                                        // int64 half-edges before loop l
             {4, t},                                        // fp32 perimeter
             {12, t},                                       // fp32 x 3 centroid
             {1, nm_scan_bytes(3 * T)},                     // tile sums of the two scans, one after the other
             {8, 2}}, {}};                                  // int64 L and B' as the scans gave them
}
static inline bool nl_totals_ok(i64 T, i64 L, i64 B) { return L >= 0 && B >= 0 && L <= T && B <= 3 * T; }
// rounds of pointer doubling that reach around a cycle of up to B half-edges: ceil(log2 B) + 1
static inline int nl_rounds(i64 B) {
    int r = 1;
    for (i64 reach = 1; reach < B; reach *= 2) ++r;
    return r;
}

// ---- mesh edges: nfl_mesh_fill_count / nfl_mesh_fill_emit
enum { NF_LEN, NF_NV, NF_VOFF, NF_NT, NF_TOFF, NF_SUMS, NF_REGIONS };
static inline NgLayout<NF_REGIONS> nf_layout(i64 L) {
    const size_t l = (size_t)L;
    return {{{4, l},                                        // int32 length of a selected loop, 0: not selected
             {4, l},                                        // int32 new vertices of loop l: 0 or 1
             {8, l},                                        // int64 new vertices before loop l
             {4, l},                                        // int32 new triangles of loop l
             {8, l},                                        // int64 new triangles before loop l
             {1, nm_scan_bytes(L)}}, {}};                   // tile sums of the two scans, one after the other
}
static inline bool nf_totals_ok(i64 L, i64 B, i64 nv, i64 nt) { return nv >= 0 && nt >= 0 && nv <= L && nt <= B; }
