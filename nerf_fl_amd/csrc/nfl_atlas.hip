// nfl_atlas.hip -- a texture atlas for a mesh (include/nerf_fl_amd.h, "mesh atlas"): one chart per triangle, two triangles
// to a square cell of C x C texels, all cells the same size.  DESIGN.md section 28.
//
// Points.   A thread per texel of the range: its cell, half and barycentrics by integer arithmetic (three 32-bit divisions a
//           thread, by W and by C; there is no loop to keep them out of), the interpolated position and the normalised
//           interpolated normal of its triangle.  The texels are what nfl_mesh_blend then takes for "vertices".
// Resolve.  A thread per texel of the range: the blend's sums into a colour, the fallback for an unseen texel, the background
//           for one without an owner.
// Shade.    nfl_mesh_shade's thread per word over the same front (nfl_meshray.h: the search, and u, v and the distance
//           recomputed through nmc_ray<false>) and the same four outputs; the colour is a bilinear lookup in the triangle's
//           half-cell.  The cell's integer origin is added after the floor, never in floating point.
//
// The rows of three floats that points and resolve write go out through LDS: a lane that stored its own row would write 4 of
// every 12 bytes of the wave's span per instruction; staged, consecutive lanes store consecutive words.  The stride of 3 words
// is odd, so the staging writes meet no bank twice.  No scratch, no atomics, the same bits every time.
#include <math.h>

#include "nfl_geom.h"
#include "nfl_meshray.h"
#include "nfl_pixel.h"

#define NA_MIN_CELL 6
#define NA_MAX_CELL 1024

// Texel e of an atlas `cols` cells of C texels wide: its triangle 2 k + h and its (extrapolated, never clamped) barycentrics
NFL_DEV void na_texel(unsigned e, int C, int cols, i64& tr, float& u, float& v) {
    const unsigned W = (unsigned)cols * (unsigned)C;
    const unsigned Y = e / W, X = e - Y * W;
    const unsigned cy = Y / (unsigned)C, cx = X / (unsigned)C;
    const int i = (int)(X - cx * (unsigned)C), j = (int)(Y - cy * (unsigned)C);
    const int h = i + j <= C - 1 ? 0 : 1;
    tr = 2 * ((i64)cy * cols + cx) + h;
    const float L = (float)(C - 5);
    u = (float)(h ? (C - 2) - i : i - 1) / L;
    v = (float)(h ? (C - 2) - j : j - 1) / L;
}

// the three indices of triangle tr when it owns its texels: tr < T and every index inside [0, V)
NFL_DEV bool na_owner(const int32_t* tri, i64 tr, i64 T, i64 V, int32_t idx[3]) {
    if (tr >= T) return false;
    idx[0] = tri[3 * tr], idx[1] = tri[3 * tr + 1], idx[2] = tri[3 * tr + 2];
    return nm_in_range(idx[0], idx[1], idx[2], V);
}

// Rows row0 .. row0 + rows - 1 of `out` (three floats each), one from every thread of the workgroup below `rows`, through
// `stage` (3 * NM_THREADS floats of LDS).  Every thread of the workgroup calls.
NFL_DEV void na_store_rows(float* out, i64 row0, int rows, const float r[3], float* stage) {
    const int t = threadIdx.x;
    __syncthreads();                                        // the call before this one is still reading the stage
    stage[3 * t] = r[0], stage[3 * t + 1] = r[1], stage[3 * t + 2] = r[2];
    __syncthreads();
    for (int k = t; k < 3 * rows; k += NM_THREADS) out[3 * row0 + k] = stage[k];
}

__global__ __launch_bounds__(NM_THREADS) void nfl_atlas_points_kernel(const nfl_atlas_points_args a) {
    __shared__ float stage[3 * NM_THREADS];
    const i64 row0 = (i64)blockIdx.x * NM_THREADS, n = row0 + threadIdx.x;
    const i64 left = a.n_texels - row0;
    const int rows = left < NM_THREADS ? (int)left : NM_THREADS;
    const float nan = __builtin_nanf("");
    float p[3] = {nan, nan, nan}, m[3] = {0.f, 0.f, 0.f};
    if (n < a.n_texels) {
        i64 tr;
        float u, v;
        int32_t idx[3];
        na_texel((unsigned)(a.first_texel + n), a.cell, a.cols, tr, u, v);
        if (na_owner(a.d_triangles, tr, a.n_triangles, a.n_vertices, idx)) {
            const float w0 = (1.f - u) - v;
            const float *A = a.d_vertices + 3 * (i64)idx[0], *B = a.d_vertices + 3 * (i64)idx[1], *Cc = a.d_vertices + 3 * (i64)idx[2];
            const float *NA = a.d_vertex_normals + 3 * (i64)idx[0], *NB = a.d_vertex_normals + 3 * (i64)idx[1],
                        *NC = a.d_vertex_normals + 3 * (i64)idx[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = nmc_mix(w0, u, v, A[k], B[k], Cc[k]), m[k] = nmc_mix(w0, u, v, NA[k], NB[k], NC[k]);
            const float len = sqrtf(nmc_dot(m[0], m[1], m[2], m[0], m[1], m[2]));
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] = len > 0.f ? m[k] / len : 0.f;                     // 0 or NaN: no normal
        }
    }
    na_store_rows(a.d_points, row0, rows, p, stage);
    na_store_rows(a.d_normals, row0, rows, m, stage);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_atlas_resolve_kernel(const nfl_atlas_resolve_args a) {
    __shared__ float stage[3 * NM_THREADS];
    const i64 row0 = (i64)blockIdx.x * NM_THREADS, n = row0 + threadIdx.x;
    const i64 left = a.n_texels - row0;
    const int rows = left < NM_THREADS ? (int)left : NM_THREADS;
    float c[3] = {a.background[0], a.background[1], a.background[2]};
    bool seen = false;
    if (n < a.n_texels) {
        i64 tr;
        float u, v;
        int32_t idx[3];
        na_texel((unsigned)(a.first_texel + n), a.cell, a.cols, tr, u, v);
        if (na_owner(a.d_triangles, tr, a.n_triangles, a.n_vertices, idx)) {
            seen = a.d_views[n] > 0;
            if (seen) {
                const float4 s = reinterpret_cast<const float4*>(a.d_sum)[n];
                c[0] = fminf(fmaxf(s.x / s.w, 0.f), 1.f), c[1] = fminf(fmaxf(s.y / s.w, 0.f), 1.f), c[2] = fminf(fmaxf(s.z / s.w, 0.f), 1.f);
            } else if (a.d_vertex_colors) {
                const float w0 = (1.f - u) - v;
                const float *A = a.d_vertex_colors + 3 * (i64)idx[0], *B = a.d_vertex_colors + 3 * (i64)idx[1],
                            *Cc = a.d_vertex_colors + 3 * (i64)idx[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = nmc_mix(w0, u, v, A[k], B[k], Cc[k]);
            } else {
                c[0] = a.fallback[0], c[1] = a.fallback[1], c[2] = a.fallback[2];
            }
        }
        if (a.d_texture_u8) a.d_texture_u8[3 * n] = nmc_byte(c[0]), a.d_texture_u8[3 * n + 1] = nmc_byte(c[1]), a.d_texture_u8[3 * n + 2] = nmc_byte(c[2]);
        if (a.d_seen) a.d_seen[n] = seen ? 1 : 0;
    }
    if (a.d_texture) na_store_rows(a.d_texture, row0, rows, c, stage);                  // uniform over the workgroup
}

// texel (x, y) of the atlas, W texels wide
NFL_DEV void na_fetch(const nfl_mesh_shade_atlas_args& a, i64 W, int x, int y, float c[3]) {
    const i64 at = 3 * ((i64)y * W + x);
    if (a.d_atlas) {
        c[0] = a.d_atlas[at], c[1] = a.d_atlas[at + 1], c[2] = a.d_atlas[at + 2];
    } else {
        c[0] = (float)a.d_atlas_u8[at] / 255.0f, c[1] = (float)a.d_atlas_u8[at + 1] / 255.0f, c[2] = (float)a.d_atlas_u8[at + 2] / 255.0f;
    }
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_shade_atlas_kernel(const nfl_mesh_shade_atlas_args a) {
    const i64 w = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (w >= a.n_vis) return;
    float rgb[3] = {a.background[0], a.background[1], a.background[2]};
    float depth = __builtin_huge_valf();
    int32_t winner = -1;
    NmcCovered c;
    if (nmc_covered(a, w, c)) {
        depth = c.d, winner = (int32_t)c.tr;
        // the triangle's half-cell: tr < T <= 2 cols rows, so the cell lies inside the atlas
        const int C = a.cell, cell = (int)(c.tr >> 1);
        const int cy = cell / a.cols, cx = cell - cy * a.cols;
        const float L = (float)(C - 5), last = (float)(C - 1);
        float lx = 1.f + c.u * L, ly = 1.f + c.v * L;
        if (c.tr & 1) lx = last - lx, ly = last - ly;
        lx = fminf(fmaxf(lx, 0.f), last), ly = fminf(fmaxf(ly, 0.f), last);            // NaN -> 0: forged words stay in the cell
        const float xf = floorf(lx), yf = floorf(ly), tx = lx - xf, ty = ly - yf, sx = 1.f - tx, sy = 1.f - ty;
        const int xa = (int)xf, ya = (int)yf;
        const int xb = xa + 1 < C ? xa + 1 : C - 1, yb = ya + 1 < C ? ya + 1 : C - 1;
        const int ox = cx * C, oy = cy * C;
        const i64 W = (i64)a.cols * C;
        float c00[3], c10[3], c01[3], c11[3];
        na_fetch(a, W, ox + xa, oy + ya, c00);
        na_fetch(a, W, ox + xb, oy + ya, c10);
        na_fetch(a, W, ox + xa, oy + yb, c01);
        na_fetch(a, W, ox + xb, oy + yb, c11);
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = nmc_bilinear(c00[k], c10[k], c01[k], c11[k], sx, tx, sy, ty);
    }
    nmc_shade_out(a, w, rgb, depth, winner);
}

// ---- host ------------------------------------------------------------------------------------------------------------------

// the atlas of a mesh of T triangles; *texels = W * H
static bool na_layout_ok(int32_t C, int32_t cols, int32_t rows, i64 T, i64* texels) {
    if (C < NA_MIN_CELL || C > NA_MAX_CELL || cols < 1 || rows < 1) return false;
    const i64 W = (i64)cols * C, H = (i64)rows * C;
    if (W > INT32_MAX || H > INT32_MAX || W * H > INT32_MAX) return false;
    *texels = W * H;
    return 2 * (i64)cols * rows >= T;
}

static bool na_range_ok(i64 first, i64 n, i64 texels) { return first >= 0 && n >= 0 && first <= texels && n <= texels - first; }

extern "C" int nfl_atlas_points(const nfl_atlas_points_args* a, void* stream) {
    i64 texels = 0;
    if (!a || !nmc_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (a->n_vertices && ng_bad(a->d_vertex_normals, 4)) return NFL_EINVAL;
    if (!na_layout_ok(a->cell, a->cols, a->rows, a->n_triangles, &texels)) return NFL_EINVAL;
    if (!na_range_ok(a->first_texel, a->n_texels, texels)) return NFL_EINVAL;
    if (a->n_texels == 0) return NFL_OK;
    if (ng_bad(a->d_points, 4) || ng_bad(a->d_normals, 4)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_atlas_points_kernel, dim3(nm_grid(a->n_texels)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

extern "C" int nfl_atlas_resolve(const nfl_atlas_resolve_args* a, void* stream) {
    i64 texels = 0;
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (a->n_triangles && ng_bad(a->d_triangles, 4)) return NFL_EINVAL;
    if (!na_layout_ok(a->cell, a->cols, a->rows, a->n_triangles, &texels)) return NFL_EINVAL;
    if (!na_range_ok(a->first_texel, a->n_texels, texels)) return NFL_EINVAL;
    if (ng_misaligned(a->d_vertex_colors, 4) || ng_misaligned(a->d_texture, 4)) return NFL_EINVAL;
    if (a->n_texels == 0) return NFL_OK;
    if (ng_bad(a->d_sum, 16) || ng_bad(a->d_views, 4)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_atlas_resolve_kernel, dim3(nm_grid(a->n_texels)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

extern "C" int nfl_mesh_shade_atlas(const nfl_mesh_shade_atlas_args* a, void* stream) {
    i64 texels = 0;
    if (!a || !nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (!nmc_words_ok(a->d_vis, a->n_vis, 8)) return NFL_EINVAL;
    if (!nmc_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!na_layout_ok(a->cell, a->cols, a->rows, a->n_triangles, &texels)) return NFL_EINVAL;
    if ((a->d_atlas != nullptr) == (a->d_atlas_u8 != nullptr)) return NFL_EINVAL;      // exactly one of the two
    if (ng_misaligned(a->d_atlas, 4) || ng_misaligned(a->d_rgb, 4) || ng_misaligned(a->d_depth, 4) ||
        ng_misaligned(a->d_triangle, 4)) return NFL_EINVAL;
    if (a->n_vis == 0) return NFL_OK;
    hipLaunchKernelGGL(nfl_mesh_shade_atlas_kernel, dim3(nm_grid(a->n_vis)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
