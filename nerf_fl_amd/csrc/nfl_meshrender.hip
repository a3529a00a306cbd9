// nfl_meshrender.hip -- render a coloured mesh to images (include/nerf_fl_amd.h, "mesh render"): a visibility buffer of the
// mesh per camera (fill + raster) and a shading pass that interpolates vertex attributes at the winning triangle of every
// pixel.  DESIGN.md section 27.
//
// Fill.    A thread per word of the run: 2^64 - 1.
// Raster.  The walk of nfl_meshray.h, shared with the depth map of nfl_meshcolor.hip, so the two cannot disagree about a box
//          or a hit.  A hit is a 64-bit atomicMin of (bits(distance) << 32) | triangle: the distance decides, the lower index
//          wins a tie, and the result does not depend on the order of the hits.
// Shade.   A thread per word.  nfl_meshray.h's front gives it "uncovered", or its image, pixel and triangle with u, v and the
//          distance recomputed by the raster's own expressions; the kernel here only interpolates in one of three modes.
#include <math.h>

#include "nfl_geom.h"
#include "nfl_meshray.h"

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_visibility_fill_kernel(unsigned long long* vis, i64 n) {
    nmc_fill(vis, n, NMR_EMPTY);
}

struct NmrVisibilitySink {
    unsigned long long* vis;
    NFL_DEV void hit(float d, int tri, i64 w) const {
        if (!(d < __builtin_huge_valf())) return;           // an overflowed distance is no hit: 2^64 - 1 stays "nothing"
        atomicMin(vis + w, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)tri);
    }
};

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_visibility_raster_kernel(const nfl_mesh_visibility_args a) {
    nmc_raster(a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles, a.d_table, a.first, a.count, a.n_vis,
               NmrVisibilitySink{reinterpret_cast<unsigned long long*>(a.d_vis)});
}

extern "C" int nfl_mesh_visibility(const nfl_mesh_visibility_args* a, void* stream) {
    if (!a || !nmc_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (!nmc_words_ok(a->d_vis, a->n_vis, 8)) return NFL_EINVAL;
    const i64 items = a->n_triangles * a->count;
    if (ng_cdiv(items, NM_THREADS) > INT32_MAX) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->n_vis)
        hipLaunchKernelGGL(nfl_mesh_visibility_fill_kernel, dim3(nm_grid(a->n_vis)), dim3(NM_THREADS), 0, s,
                           reinterpret_cast<unsigned long long*>(a->d_vis), a->n_vis);
    if (items && a->n_vertices && a->n_vis)
        hipLaunchKernelGGL(nfl_mesh_visibility_raster_kernel, dim3(nm_grid(items)), dim3(NM_THREADS), 0, s, *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---- shade -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_shade_kernel(const nfl_mesh_shade_args a) {
    const i64 w = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (w >= a.n_vis) return;
    float rgb[3] = {a.background[0], a.background[1], a.background[2]};
    float depth = __builtin_huge_valf();
    int32_t winner = -1;
    NmcCovered c;
    if (nmc_covered(a, w, c)) {
        depth = c.d, winner = (int32_t)c.tr;
        if (a.mode == NFL_SHADE_FACING) {
            const nfl_image_rec& im = *c.im;
            const NmcTri& t = c.t;
            const float dx = ((float)c.i - im.cx) / im.fx, dy = -((float)c.j - im.cy) / im.fy, dz = -1.f;
            const float n0 = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1], n1 = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2],
                        n2 = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
            float g = fabsf(nmc_dot(n0, n1, n2, dx, dy, dz)) / (sqrtf(nmc_dot(n0, n1, n2, n0, n1, n2)) * sqrtf(nmc_dot(dx, dy, dz, dx, dy, dz)));
            if (!(g == g)) g = 0.f;
            rgb[0] = rgb[1] = rgb[2] = g;
        } else {
            const float w0 = (1.f - c.u) - c.v;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                rgb[k] = nmc_mix(w0, c.u, c.v, a.d_attr[3 * (i64)c.idx[0] + k], a.d_attr[3 * (i64)c.idx[1] + k], a.d_attr[3 * (i64)c.idx[2] + k]);
            if (a.mode == NFL_SHADE_NORMAL) {
                const float len = sqrtf(nmc_dot(rgb[0], rgb[1], rgb[2], rgb[0], rgb[1], rgb[2]));
#pragma unroll
                for (int k = 0; k < 3; ++k) rgb[k] = len > 0.f ? 0.5f * (rgb[k] / len) + 0.5f : 0.5f;      // 0 or NaN: grey
            }
        }
    }
    nmc_shade_out(a, w, rgb, depth, winner);
}

extern "C" int nfl_mesh_shade(const nfl_mesh_shade_args* a, void* stream) {
    if (!a || !nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (a->mode != NFL_SHADE_COLOR && a->mode != NFL_SHADE_NORMAL && a->mode != NFL_SHADE_FACING) return NFL_EINVAL;
    if (!nmc_words_ok(a->d_vis, a->n_vis, 8)) return NFL_EINVAL;
    if (!nmc_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (a->mode != NFL_SHADE_FACING && a->n_vertices && !a->d_attr) return NFL_EINVAL;
    if (ng_misaligned(a->d_attr, 4) || ng_misaligned(a->d_rgb, 4) || ng_misaligned(a->d_depth, 4) ||
        ng_misaligned(a->d_triangle, 4)) return NFL_EINVAL;
    if (a->n_vis == 0) return NFL_OK;
    hipLaunchKernelGGL(nfl_mesh_shade_kernel, dim3(nm_grid(a->n_vis)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
