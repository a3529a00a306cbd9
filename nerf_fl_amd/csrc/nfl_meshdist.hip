// nfl_meshdist.hip -- the distance between triangle meshes on the device (include/nerf_fl_amd.h, "mesh distance"): a uniform
// grid of triangle lists, the closest point of a mesh for many queries (through the grid, or trying every triangle), area-
// weighted samples of a surface, and the reduction of a run of distances.  DESIGN.md section 33.
//
//   grid     count   zero; a thread per triangle adds 1 to every cell of its index box (int32 atomics); nm_scan: the rows' offsets
//            emit    the offsets (cells + 1), the cursors = 0; a thread per triangle writes itself into its rows at the place
//                    the cell's cursor hands out (the order of arrival: arbitrary, and nothing reads a row for its order)
//   closest  a thread per query.  Brute: the workgroup stages 256 triangles' corners in LDS (nine planes of 256 floats and a
//            flag, so the 64 lanes of a wave read ONE word each step: a broadcast) and every thread tries them all.  Grid: the
//            thread walks the shells of cells round its own and stops on the bound of the header; neighbouring queries
//            (samples lie in triangle order) walk neighbouring rows, which is what the caches are for.
//   samples  count   a thread per triangle: m_t; nm_scan: the first row of every triangle
//            emit    a thread per triangle writes up to 64 samples itself; the wave then takes the larger triangles of its
//                    lanes one after the other, 64 samples a step (nfl_mesh_depth's treatment of large boxes)
//   reduce   the library's fixed-order fp64 reduction (nfl_reduce.h); here only its policy: what a distance adds to the columns
//
// The triangle fetch (nm_corners), the face normal (nm_face_cross), the hash (ng_mix) and the finite test are nfl_geom.h's,
// the pointer checks nfl_geom_layout.h's: registration and the sampler read a triangle exactly as nfl_mesh_closest does.
// The view of a mesh with its grid, the read of a row and brute mode's staged tiles are nfl_trigrid.h's, shared with nfl_meshcast.
//
// Only integer atomics, and nothing that depends on their order leaves a call except the order inside a grid row.  Nothing
// here allocates, sets or copies memory through the runtime.
#include <math.h>

#include "nfl_reduce.h"
#include "nfl_trigrid.h"

typedef unsigned long long u64;

#define ND_WAVE_SAMPLES 64                                  // a triangle with more samples is emitted by the whole wave

#ifdef NFL_MESHDIST_COUNT_TESTS
// a diagnostic build (make variant VFLAGS=-DNFL_MESHDIST_COUNT_TESTS=1 VTU=nfl_meshdist) counts what the grid walk does:
// [0] point-triangle tests, [1] cells read, [2] queries.  tests/time_meshdist.py reads them; the product never has them.
__device__ u64 nd_debug_counts[3];
extern "C" int nfl_meshdist_debug_counts(u64* out3, int reset) {
    const u64 zero[3] = {0, 0, 0};
    if (out3 && hipMemcpyFromSymbol(out3, HIP_SYMBOL(nd_debug_counts), sizeof zero) != hipSuccess) return NFL_ELAUNCH;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(nd_debug_counts), zero, sizeof zero) != hipSuccess) return NFL_ELAUNCH;
    return NFL_OK;
}
#define ND_DEBUG_ADD(k, n) atomicAdd(&nd_debug_counts[k], (u64)(n))
#else
#define ND_DEBUG_ADD(k, n)
#endif

// ---------------------------------------------------------------------------------------------------------- device pieces
// (the grid itself -- NdGrid, nd_grid_ok, nd_grid_of, nd_cellf, nd_face -- is nfl_geom.h's: nfl_meshcast walks the same cells)

__device__ __forceinline__ float nd_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the index box of a usable triangle
__device__ __forceinline__ void nd_box(const NdGrid& G, const float* a, const float* b, const float* c, int* i0, int* i1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        i0[k] = nd_cellf(fminf(fminf(a[k], b[k]), c[k]), G.lo[k], G.cell, G.dims[k]);
        i1[k] = nd_cellf(fmaxf(fmaxf(a[k], b[k]), c[k]), G.lo[k], G.cell, G.dims[k]);
    }
}

// POINT AND TRIANGLE of the header: q, (u, v, w) and dd for the query p.  The regions and the parameters in fp64 -- the
// 2 x 2 determinants cancel, and in fp32 a sliver of marching tetrahedra put q 3e-6 from a point that lay ON it -- q rounded
// to fp32, clamped, and the distance in fp32
__device__ __forceinline__ double nd_dot64(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ float nd_point_triangle(const float* p, const float* a, const float* b, const float* c, float* q,
                                                   float* uvw) {
    double ab[3], ac[3], bc[3], ap[3], bp[3], cp[3], A[3], B[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = (double)a[k], B[k] = (double)b[k];
        ab[k] = B[k] - A[k];
        ac[k] = (double)c[k] - A[k];
        bc[k] = (double)c[k] - B[k];
        ap[k] = (double)p[k] - A[k];
        bp[k] = (double)p[k] - B[k];
        cp[k] = (double)p[k] - (double)c[k];
    }
    const double d1 = nd_dot64(ab, ap), d2 = nd_dot64(ac, ap), d3 = nd_dot64(ab, bp), d4 = nd_dot64(ac, bp);
    const double d5 = nd_dot64(ab, cp), d6 = nd_dot64(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double u, v, w, Q[3];
    if (d1 <= 0.0 && d2 <= 0.0) {
        u = 1.0, v = 0.0, w = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[k] = A[k];
    } else if (d3 >= 0.0 && d4 <= d3) {
        u = 0.0, v = 1.0, w = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[k] = B[k];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double s = d1 / (d1 - d3);
        u = 1.0 - s, v = s, w = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[k] = A[k] + s * ab[k];
    } else if (d6 >= 0.0 && d5 <= d6) {
        u = 0.0, v = 0.0, w = 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[k] = (double)c[k];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double s = d2 / (d2 - d6);
        u = 1.0 - s, v = 0.0, w = s;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[k] = A[k] + s * ac[k];
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double s = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        u = 0.0, v = 1.0 - s, w = s;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[k] = B[k] + s * bc[k];
    } else {
        const double den = 1.0 / ((va + vb) + vc), s = vb * den, r = vc * den;
        u = (1.0 - s) - r, v = s, w = r;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[k] = (A[k] + s * ab[k]) + r * ac[k];
    }
    uvw[0] = (float)u, uvw[1] = (float)v, uvw[2] = (float)w;
    float e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float mn = fminf(fminf(a[k], b[k]), c[k]), mx = fmaxf(fmaxf(a[k], b[k]), c[k]);
        q[k] = (float)Q[k];
        q[k] = q[k] < mn ? mn : (q[k] > mx ? mx : q[k]);                // a NaN stays
        e[k] = p[k] - q[k];
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// the best candidate of a query so far
struct NdBest {
    float dd;
    int32_t t;
    float q[3], uvw[3];
};

__device__ __forceinline__ void nd_try(NdBest& B, const float* p, int32_t t, const float* a, const float* b, const float* c,
                                       float limit) {
    float q[3], uvw[3];
    const float dd = nd_point_triangle(p, a, b, c, q, uvw);
    if (dd <= limit && dd < INFINITY && (dd < B.dd || (dd == B.dd && t < B.t))) {
        B.dd = dd;
        B.t = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) B.q[k] = q[k], B.uvw[k] = uvw[k];
    }
}

// --------------------------------------------------------------------------------------------------------------- the grid

extern "C" size_t nfl_trigrid_bytes(int32_t nx, int32_t ny, int32_t nz) {
    const int32_t dims[3] = {nx, ny, nz};
    if (!nd_dims_ok(dims)) return 0;
    return ng_bytes(nd_grid_layout((i64)nx * ny * nz));
}

typedef NgLayout<ND_G_REGIONS> NdGridScratch;

static int nd_grid_carve(const nfl_trigrid_args* a, NdGridScratch& S) {
    if (!a || !nd_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!nd_grid_ok(a->lo, a->cell, a->dims)) return NFL_EINVAL;
    S = nd_grid_layout((i64)a->dims[0] * a->dims[1] * a->dims[2]);
    return ng_carve(S, a->d_scratch, a->scratch_bytes);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_trigrid_zero_kernel(int32_t* cnt, i64 cells, i64* totals) {
    const i64 c = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (c < cells) cnt[c] = 0;
    if (c == 0 && totals) totals[1] = 0;
}

// FILL false: count the cells' triangles; true: write triangle t into its rows
template <bool FILL>
__global__ __launch_bounds__(NM_THREADS) void nfl_trigrid_walk_kernel(const float* ver, const int32_t* tri, i64 V, i64 T,
                                                                      const NdGrid G, int32_t* cnt, const i64* off,
                                                                      i64 n_entries, int32_t* entries, i64* n_outside) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool outside = false;
    if (t < T) {
        float a[3], b[3], c[3];
        outside = !nm_in_range(tri[3 * t], tri[3 * t + 1], tri[3 * t + 2], V);
        if (nm_corners(ver, tri, V, t, a, b, c)) {
            int i0[3], i1[3];
            nd_box(G, a, b, c, i0, i1);
            for (int z = i0[2]; z <= i1[2]; ++z)
                for (int y = i0[1]; y <= i1[1]; ++y)
                    for (int x = i0[0]; x <= i1[0]; ++x) {
                        const i64 cell = ((i64)z * G.dims[1] + y) * G.dims[0] + x;
                        const int32_t k = atomicAdd(cnt + cell, 1);
                        if (FILL) {
                            const i64 at = off[cell] + k;
                            if (k >= 0 && at >= 0 && at < n_entries) entries[at] = (int32_t)t;      // the counts of the count call put it there
                        }
                    }
        }
    }
    if (!FILL) ng_count_bad(outside, n_outside);
}

extern "C" int nfl_trigrid_count(const nfl_trigrid_args* a, void* stream) {
    NdGridScratch S;
    const int rc = nd_grid_carve(a, S);
    if (rc != NFL_OK) return rc;
    if (ng_bad(a->d_totals, 8)) return NFL_EINVAL;
    const i64 cells = (i64)a->dims[0] * a->dims[1] * a->dims[2], T = a->n_triangles;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* cnt = S.get<int32_t>(ND_G_CNT);
    hipLaunchKernelGGL(nfl_trigrid_zero_kernel, dim3(nm_grid(cells)), dim3(NM_THREADS), 0, s, cnt, cells, a->d_totals);
    if (T)
        hipLaunchKernelGGL(nfl_trigrid_walk_kernel<false>, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_vertices, a->d_triangles,
                           a->n_vertices, T, nd_grid_of(a->lo, a->cell, a->dims), cnt, nullptr, 0, nullptr, a->d_totals + 1);
    nm_scan(cnt, S.get<i64>(ND_G_OFF), cells, S.get<i64>(ND_G_SUMS), a->d_totals, s);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// thread c of cells + 1: the offset (the total at the end), and the cursor of cell c back to zero
__global__ __launch_bounds__(NM_THREADS) void nfl_trigrid_offsets_kernel(const i64* off, i64 cells, i64 n_entries, i64* out,
                                                                         int32_t* cnt) {
    const i64 c = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (c > cells) return;
    const i64 o = c < cells ? off[c] : n_entries;
    out[c] = o < 0 ? 0 : o > n_entries ? n_entries : o;
    if (c < cells) cnt[c] = 0;
}

extern "C" int nfl_trigrid_emit(const nfl_trigrid_args* a, void* stream) {
    NdGridScratch S;
    const int rc = nd_grid_carve(a, S);
    if (rc != NFL_OK) return rc;
    if (a->n_entries < 0 || a->n_entries > ND_MAX_ENTRIES) return NFL_EINVAL;
    if (ng_bad(a->d_offsets, 8)) return NFL_EINVAL;
    if (a->n_entries && ng_bad(a->d_entries, 4)) return NFL_EINVAL;
    const i64 cells = (i64)a->dims[0] * a->dims[1] * a->dims[2], T = a->n_triangles;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* cnt = S.get<int32_t>(ND_G_CNT);
    const i64* off = S.get<i64>(ND_G_OFF);
    hipLaunchKernelGGL(nfl_trigrid_offsets_kernel, dim3(nm_grid(cells + 1)), dim3(NM_THREADS), 0, s, off, cells, a->n_entries,
                       a->d_offsets, cnt);
    if (T && a->n_entries)
        hipLaunchKernelGGL(nfl_trigrid_walk_kernel<true>, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_vertices, a->d_triangles,
                           a->n_vertices, T, nd_grid_of(a->lo, a->cell, a->dims), cnt, off, a->n_entries, a->d_entries, nullptr);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------- closest point

// g * g of the header for one face: the face at index i of axis k, p beyond it by G in fp64
__device__ __forceinline__ float nd_face_bound(const NdGrid& G, int k, int i, float p, bool low_side) {
    double F, S;
    nd_face(G.lo[k], G.cell, i, &F, &S);
    double gap = low_side ? (double)p - (F + S) : (F - S) - (double)p;
    if (!(gap > 0.0)) gap = 0.0;
    const float g = (float)(gap * (1.0 - 1.1920928955078125e-07));                      // 1 - 2^-23
    return g * g;
}

__device__ __forceinline__ int nd_iabs(int x) { return x < 0 ? -x : x; }

__device__ __forceinline__ void nd_walk_grid(NdBest& B, const float* p, const NtMesh& M, float limit) {
    const NdGrid& G = M.G;
    const auto attempt = [&](int32_t t, const float* ca, const float* cb, const float* cc) NT_INLINE {
        ND_DEBUG_ADD(0, 1);
        nd_try(B, p, t, ca, cb, cc, limit);
        return false;                                                   // a closer triangle can stand anywhere in a row
    };
    const auto row = [&](i64 cell) NT_INLINE {
        ND_DEBUG_ADD(1, 1);
        nt_row(M, cell, attempt);
    };
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = nd_cellf(p[k], G.lo[k], G.cell, G.dims[k]);
    ND_DEBUG_ADD(2, 1);
    const int r_max = max(max(G.dims[0], G.dims[1]), G.dims[2]);        // the block is the whole grid by then
    for (int r = 0; r <= r_max; ++r) {
        int b0[3], b1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) b0[k] = max(c[k] - r, 0), b1[k] = min(c[k] + r, G.dims[k] - 1);
        for (int z = b0[2]; z <= b1[2]; ++z)
            for (int y = b0[1]; y <= b1[1]; ++y) {
                const i64 first = ((i64)z * G.dims[1] + y) * G.dims[0];
                if (nd_iabs(z - c[2]) == r || nd_iabs(y - c[1]) == r) {
                    for (int x = b0[0]; x <= b1[0]; ++x) row(first + x);
                } else {
                    if (c[0] - r >= 0) row(first + (c[0] - r));
                    if (r > 0 && c[0] + r < G.dims[0]) row(first + (c[0] + r));
                }
            }
        float bound = INFINITY;
        bool whole = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (b0[k] > 0) bound = fminf(bound, nd_face_bound(G, k, b0[k], p[k], true)), whole = false;
            if (b1[k] < G.dims[k] - 1) bound = fminf(bound, nd_face_bound(G, k, b1[k] + 1, p[k], false)), whole = false;
        }
        if (whole || B.dd < bound || bound > limit) return;
    }
}

// what nfl_mesh_closest asks: the queries, the limit, and where the answers go
struct NdClosest {
    NtMesh M;
    const float *points, *normals;
    i64 n;
    float max_distance;
    float* distance;
    int32_t* triangle;
    float *point, *bary, *dot;
};

template <bool GRID>
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_closest_kernel(const NdClosest a) {
    const i64 n = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    const bool mine = n < a.n;
    float p[3] = {0.f, 0.f, 0.f};
    if (mine) p[0] = a.points[3 * n], p[1] = a.points[3 * n + 1], p[2] = a.points[3 * n + 2];
    const bool asks = mine && ng_is_finite(p[0]) && ng_is_finite(p[1]) && ng_is_finite(p[2]);
    const float limit = a.max_distance * a.max_distance;
    NdBest B;
    B.dd = INFINITY, B.t = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) B.q[k] = B.uvw[k] = NAN;
    if (GRID) {
        if (asks) nd_walk_grid(B, p, a.M, limit);
    } else {
        const auto still = [&]() NT_INLINE { return asks; };
        const auto attempt = [&](int32_t t, const float* ta, const float* tb, const float* tc) NT_INLINE {
            nd_try(B, p, t, ta, tb, tc, limit);
        };
        nt_tiles(a.M, still, attempt);
    }
    if (!mine) return;
    a.distance[n] = B.t >= 0 ? sqrtf(B.dd) : INFINITY;
    a.triangle[n] = B.t;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.point[3 * n + k] = B.q[k], a.bary[3 * n + k] = B.uvw[k];
    if (a.dot) {
        float dot = NAN;
        float ca[3], cb[3], cc[3];
        if (B.t >= 0 && nm_corners(a.M.ver, a.M.tri, a.M.V, B.t, ca, cb, cc)) {
            float cr[3], len;
            nm_face_cross(ca, cb, cc, cr, &len);
            float nf[3] = {0.f, 0.f, 0.f};                              // a face without a normal: dot = 0
            if (len > 0.f) nf[0] = cr[0] / len, nf[1] = cr[1] / len, nf[2] = cr[2] / len;
            const float nq[3] = {a.normals[3 * n], a.normals[3 * n + 1], a.normals[3 * n + 2]};
            dot = nd_dot(nq, nf);
        }
        a.dot[n] = dot;
    }
}

extern "C" int nfl_mesh_closest(const nfl_mesh_closest_args* a, void* stream) {
    if (!a || a->n_points < 0 || a->n_points > ND_MAX_ENTRIES) return NFL_EINVAL;
    if (!nd_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!(a->max_distance > 0.f)) return NFL_EINVAL;                                    // NaN included
    if ((a->d_normals == nullptr) != (a->d_dot == nullptr)) return NFL_EINVAL;
    const bool grid = a->d_offsets != nullptr;                                          // without rows lo, cell, dims are not read
    if (grid && !nt_rows_ok(a->d_offsets, a->d_entries, a->n_entries, a->lo, a->cell, a->dims)) return NFL_EINVAL;
    if (a->n_points == 0) return NFL_OK;
    const void* need[] = {a->d_points, a->d_distance, a->d_triangle, a->d_point, a->d_bary};
    for (const void* p : need)
        if (ng_bad(p, 4)) return NFL_EINVAL;
    if (ng_misaligned(a->d_normals, 4) || ng_misaligned(a->d_dot, 4)) return NFL_EINVAL;
    const NdClosest q = {{a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles, a->d_offsets, a->d_entries,
                          grid ? a->n_entries : 0, nd_grid_of(a->lo, a->cell, a->dims)},
                         a->d_points, a->d_normals, a->n_points, a->max_distance, a->d_distance, a->d_triangle, a->d_point,
                         a->d_bary, a->d_dot};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (grid)
        hipLaunchKernelGGL(nfl_mesh_closest_kernel<true>, dim3(nm_grid(a->n_points)), dim3(NM_THREADS), 0, s, q);
    else
        hipLaunchKernelGGL(nfl_mesh_closest_kernel<false>, dim3(nm_grid(a->n_points)), dim3(NM_THREADS), 0, s, q);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// -------------------------------------------------------------------------------------------------------- surface samples

extern "C" size_t nfl_mesh_sample_bytes(int64_t T) {
    if (!nm_sizes_ok(0, T)) return 0;
    return ng_bytes(nd_sample_layout(T));
}

typedef NgLayout<ND_S_REGIONS> NdSampleScratch;

// Checks shared by count and emit.  NFL_OK with T == 0 means: nothing to carve.
static int nd_sample_carve(const nfl_mesh_sample_args* a, NdSampleScratch& S) {
    if (!a || !nd_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!(a->density >= 0.f) || !ng_finite(a->density)) return NFL_EINVAL;
    S = nd_sample_layout(a->n_triangles);
    if (a->n_triangles == 0) return NFL_OK;
    return ng_carve(S, a->d_scratch, a->scratch_bytes);
}

// cr and len of triangle t from its corners; the hash of the triangle
struct NdFace {
    float a[3], e1[3], e2[3], cr[3], len;
};

__device__ __forceinline__ bool nd_face(const float* ver, const int32_t* tri, i64 V, i64 t, NdFace& f) {
    float b[3], c[3];
    if (!nm_corners(ver, tri, V, t, f.a, b, c)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) f.e1[k] = b[k] - f.a[k], f.e2[k] = c[k] - f.a[k];
    nm_face_cross(f.a, b, c, f.cr, &f.len);
    return f.len > 0.f && ng_is_finite(f.len);
}

#define ND_2M24 5.9604644775390625e-08f                     // 2^-24

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_sample_count_kernel(const float* ver, const int32_t* tri, i64 V, i64 T,
                                                                           float density, u64 seed, int32_t* cnt, i64* totals) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool outside = false, dense = false;
    if (t < T) {
        outside = !nm_in_range(tri[3 * t], tri[3 * t + 1], tri[3 * t + 2], V);
        NdFace f;
        int32_t m = 0;
        if (nd_face(ver, tri, V, t, f)) {
            const u64 ht = ng_mix(ng_mix(seed) + (u64)t);
            const float ut = (float)(ht >> 40) * ND_2M24;
            const float x = (0.5f * f.len) * density + ut;
            dense = !(x < ND_MAX_SAMPLES_PER_TRIANGLE);
            m = dense ? 0 : (int32_t)floorf(x);
        }
        cnt[t] = m;
    }
    ng_count_bad(outside, totals + 1);
    ng_count_bad(dense, totals + 2);
}

__global__ __launch_bounds__(64) void nfl_mesh_sample_zero_kernel(i64* totals) {
    if (threadIdx.x < 3) totals[threadIdx.x] = 0;
}

extern "C" int nfl_mesh_sample_count(const nfl_mesh_sample_args* a, void* stream) {
    NdSampleScratch S;
    const int rc = nd_sample_carve(a, S);
    if (rc != NFL_OK) return rc;
    if (ng_bad(a->d_totals, 8)) return NFL_EINVAL;
    const i64 T = a->n_triangles;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nfl_mesh_sample_zero_kernel, dim3(1), dim3(64), 0, s, a->d_totals);
    if (T) {
        int32_t* cnt = S.get<int32_t>(ND_S_CNT);
        hipLaunchKernelGGL(nfl_mesh_sample_count_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_vertices, a->d_triangles,
                           a->n_vertices, T, a->density, a->seed, cnt, a->d_totals);
        nm_scan(cnt, S.get<i64>(ND_S_OFF), T, S.get<i64>(ND_S_SUMS), a->d_totals, s);
    }
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// sample j of triangle t to row `at`
__device__ __forceinline__ void nd_emit_sample(const nfl_mesh_sample_args& a, const NdFace& f, u64 ht, i64 t, int32_t j, i64 at) {
    if (at < 0 || at >= a.n_samples) return;
    const u64 hj = ng_mix(ht + (u64)(j + 1));
    float r1 = ((float)(hj >> 40) + 0.5f) * ND_2M24, r2 = ((float)((hj >> 16) & 0xFFFFFFull) + 0.5f) * ND_2M24;
    if (r1 + r2 > 1.f) r1 = 1.f - r1, r2 = 1.f - r2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.d_points[3 * at + k] = (f.a[k] + r1 * f.e1[k]) + r2 * f.e2[k];
        a.d_normals[3 * at + k] = f.cr[k] / f.len;
    }
    a.d_sample_triangles[at] = (int32_t)t;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_sample_emit_kernel(const nfl_mesh_sample_args a, const int32_t* cnt,
                                                                          const i64* off) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t m = 0;
    i64 o = 0;
    NdFace f;
    u64 ht = 0;
    if (t < a.n_triangles) {
        m = cnt[t];
        o = off[t];
        if (m < 0 || m > (int32_t)ND_MAX_SAMPLES_PER_TRIANGLE || !nd_face(a.d_vertices, a.d_triangles, a.n_vertices, t, f)) m = 0;
        ht = ng_mix(ng_mix(a.seed) + (u64)t);
    }
    if (m <= ND_WAVE_SAMPLES)
        for (int32_t j = 0; j < m; ++j) nd_emit_sample(a, f, ht, t, j, o + j);
    // the larger triangles of the wave's lanes, one after the other, every lane 1 / 64 of the samples
    u64 todo = __ballot(m > ND_WAVE_SAMPLES);
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const i64 wt = t - lane + src;                                  // that lane's triangle
        const int32_t wm = __shfl(m, src);
        const i64 wo = __shfl(o, src);
        NdFace wf;
        if (!nd_face(a.d_vertices, a.d_triangles, a.n_vertices, wt, wf)) continue;     // the same for every lane
        const u64 wh = ng_mix(ng_mix(a.seed) + (u64)wt);
        for (int32_t j = lane; j < wm; j += 64) nd_emit_sample(a, wf, wh, wt, j, wo + j);
    }
}

extern "C" int nfl_mesh_sample_emit(const nfl_mesh_sample_args* a, void* stream) {
    NdSampleScratch S;
    const int rc = nd_sample_carve(a, S);
    if (rc != NFL_OK) return rc;
    if (a->n_samples < 0 || a->n_samples > ND_MAX_ENTRIES) return NFL_EINVAL;
    if (a->n_samples == 0 || a->n_triangles == 0) return NFL_OK;
    const void* need[] = {a->d_points, a->d_sample_triangles, a->d_normals};
    for (const void* p : need)
        if (ng_bad(p, 4)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_mesh_sample_emit_kernel, dim3(nm_grid(a->n_triangles)), dim3(NM_THREADS), 0,
                       static_cast<hipStream_t>(stream), *a, S.get<int32_t>(ND_S_CNT), S.get<i64>(ND_S_OFF));
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ------------------------------------------------------------------------------------------------------------- reduction

extern "C" size_t nfl_meshdist_reduce_bytes(int64_t n) {
    if (n < 0 || n > ND_MAX_ENTRIES) return 0;
    return ng_bytes(nd_reduce_layout(n));
}

// the reduction's policy (nfl_reduce.h): every column of the row is a thread's, NFL_MESHDIST_MAX combines by fmax
struct NdReduce {
    nfl_meshdist_reduce_args a;
    static constexpr int cols = NFL_MESHDIST_COLUMNS, width = NFL_MESHDIST_COLUMNS;
    __host__ __device__ static constexpr int column(int k) { return k; }
    struct Combine {
        __device__ __forceinline__ double operator()(int k, double x, double y) const {
            return k == NFL_MESHDIST_MAX ? fmax(x, y) : x + y;
        }
    };
    __device__ __forceinline__ void add(i64 i, double* acc) const {
        const float d = a.d_distance[i];
        if (!(d < INFINITY)) return;                                    // +inf and NaN: missing
        const double x = (double)d;
        acc[NFL_MESHDIST_COUNT] += 1.0;
        acc[NFL_MESHDIST_SUM] += x;
        acc[NFL_MESHDIST_SUM_SQ] += x * x;
        acc[NFL_MESHDIST_MAX] = fmax(acc[NFL_MESHDIST_MAX], x);
#pragma unroll
        for (int k = 0; k < NFL_MESHDIST_MAX_TAU; ++k)
            if (k < a.n_tau && d <= a.tau[k]) acc[NFL_MESHDIST_WITHIN + k] += 1.0;
        if (a.d_dot) acc[NFL_MESHDIST_SUM_DOT] += fabs((double)a.d_dot[i]);
    }
};

extern "C" int nfl_meshdist_reduce(const nfl_meshdist_reduce_args* a, void* stream) {
    if (!a || a->n < 0 || a->n > ND_MAX_ENTRIES || ng_bad(a->d_row, 8)) return NFL_EINVAL;
    if (a->n_tau < 0 || a->n_tau > NFL_MESHDIST_MAX_TAU) return NFL_EINVAL;
    for (int k = 0; k < a->n_tau; ++k)
        if (a->tau[k] != a->tau[k]) return NFL_EINVAL;
    if (a->n && ng_bad(a->d_distance, 4)) return NFL_EINVAL;
    if (ng_misaligned(a->d_dot, 4)) return NFL_EINVAL;
    double* parts = nullptr;
    const i64 blocks = nd_reduce_blocks(a->n);
    if (blocks) {
        NgLayout<ND_R_REGIONS> S = nd_reduce_layout(a->n);
        const int rc = ng_carve(S, a->d_scratch, a->scratch_bytes);
        if (rc != NFL_OK) return rc;
        parts = S.get<double>(ND_R_PARTS);
    }
    ng_reduce_launch(NdReduce{*a}, a->n, blocks, parts, a->d_row, static_cast<hipStream_t>(stream));
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
