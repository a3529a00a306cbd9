// nfl_meshcolor.hip -- colour a mesh from the images that see it (include/nerf_fl_amd.h, "mesh colour"): a depth map of the
// mesh per camera (fill + raster) and a blend of the bank's pixels into per-vertex accumulators.  DESIGN.md section 25.
//
// Fill.    A thread per depth word of the run: +inf.
// Raster.  The walk of nfl_meshray.h, shared with the visibility buffer of nfl_meshrender.hip: a thread per (triangle, image)
//          of the run, small boxes by their own lane, larger ones by the whole wave.  A hit is an atomicMin on the depth word
//          as uint32: the depths are non-negative floats, which order as their bits, and +inf is the largest.  The triangle
//          number that the walk carries is not used here.
// Blend.   A thread per vertex, the image loop inside: the records are read by every thread in the same order and stay in
//          cache; per contributing image 4 pixels through nfl_pixel_rgb and one depth word.  The thread owns its row of the
//          accumulators: no atomics, the same bits every time.
#include <math.h>

#include "nfl_geom.h"
#include "nfl_meshray.h"
#include "nfl_pixel.h"

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_depth_fill_kernel(float* depth, i64 n) {
    nmc_fill(depth, n, __builtin_huge_valf());
}

struct NmcDepthSink {
    unsigned int* depth;
    NFL_DEV void hit(float d, int, i64 w) const { atomicMin(depth + w, __float_as_uint(d)); }
};

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_depth_raster_kernel(const nfl_mesh_depth_args a) {
    nmc_raster(a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles, a.d_table, a.first, a.count, a.n_depth,
               NmcDepthSink{reinterpret_cast<unsigned int*>(a.d_depth)});
}

extern "C" int nfl_mesh_depth(const nfl_mesh_depth_args* a, void* stream) {
    if (!a || !nmc_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (!nmc_words_ok(a->d_depth, a->n_depth, 4)) return NFL_EINVAL;
    const i64 items = a->n_triangles * a->count;
    if (ng_cdiv(items, NM_THREADS) > INT32_MAX) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->n_depth) hipLaunchKernelGGL(nfl_mesh_depth_fill_kernel, dim3(nm_grid(a->n_depth)), dim3(NM_THREADS), 0, s, a->d_depth, a->n_depth);
    if (items && a->n_vertices && a->n_depth)
        hipLaunchKernelGGL(nfl_mesh_depth_raster_kernel, dim3(nm_grid(items)), dim3(NM_THREADS), 0, s, *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---- blend -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_blend_kernel(const nfl_mesh_blend_args a) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= a.n_vertices) return;
    const float p[3] = {a.d_vertices[3 * v], a.d_vertices[3 * v + 1], a.d_vertices[3 * v + 2]};
    const float nr[3] = {a.d_normals[3 * v], a.d_normals[3 * v + 1], a.d_normals[3 * v + 2]};
    const bool flat = nr[0] == 0.f && nr[1] == 0.f && nr[2] == 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int32_t views = 0;
    if (!a.start) acc = reinterpret_cast<const float4*>(a.d_sum)[v], views = a.d_views[v];
    float centre[3] = {0.f, 0.f, 0.f};
    if (a.d_center) centre[0] = a.d_center[3 * v], centre[1] = a.d_center[3 * v + 1], centre[2] = a.d_center[3 * v + 2];
    const i64 pix_first = a.count ? a.d_table[a.first].pix0 : 0;
    for (int n = a.first; n < a.first + a.count; ++n) {
        const float wi = a.d_image_weights ? a.d_image_weights[n] : 1.f;
        if (!(wi > 0.f)) continue;                                                      // 1
        const nfl_image_rec& im = a.d_table[n];
        if (im.width < 1 || im.height < 1) continue;
        float q[3];
        nmc_to_camera(im, p, q);
        const float s = -q[2];
        if (!(s > 0.f)) continue;                                                       // 2
        const float wmax = (float)(im.width - 1), hmax = (float)(im.height - 1);
        const float u = im.cx + im.fx * (q[0] / s), w = im.cy - im.fy * (q[1] / s);
        if (!(u >= 0.f && u <= wmax && w >= 0.f && w <= hmax)) continue;                // 3
        const float ex = im.c2w[3] - p[0], ey = im.c2w[7] - p[1], ez = im.c2w[11] - p[2];
        const float dist = sqrtf((ex * ex + ey * ey) + ez * ez);
        const float cosv = flat ? 1.f : nmc_dot(nr[0], nr[1], nr[2], ex, ey, ez) / dist;
        if (!(cosv > a.min_cos)) continue;                                              // 4
        const int ix = (int)floorf(u + 0.5f), iy = (int)floorf(w + 0.5f);
        const i64 word = (im.pix0 - pix_first) + (i64)iy * im.width + ix;
        if (word < 0 || word >= a.n_depth) continue;                    // a depth buffer that is not this run's: nothing read
        if (!(dist <= a.d_depth[word] + a.depth_tol)) continue;                         // 5
        const float xf = floorf(u), yf = floorf(w), tx = u - xf, ty = w - yf, sx = 1.f - tx, sy = 1.f - ty;
        const int xa = (int)xf, ya = (int)yf;
        const int xb = xa + 1 < im.width ? xa + 1 : im.width - 1, yb = ya + 1 < im.height ? ya + 1 : im.height - 1;
        float c00[3], c10[3], c01[3], c11[3], c[3];
        nfl_pixel_rgb(a.d_pixels, im, (i64)ya * im.width + xa, c00);
        nfl_pixel_rgb(a.d_pixels, im, (i64)ya * im.width + xb, c10);
        nfl_pixel_rgb(a.d_pixels, im, (i64)yb * im.width + xa, c01);
        nfl_pixel_rgb(a.d_pixels, im, (i64)yb * im.width + xb, c11);
        float off = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = nmc_bilinear(c00[k], c10[k], c01[k], c11[k], sx, tx, sy, ty);
            off = fmaxf(off, fabsf(c[k] - centre[k]));
        }
        if (a.d_center && !(off <= a.reject)) continue;                                 // 6
        const float wt = a.weighting == NFL_BLEND_COS ? wi * cosv : wi;
        acc.x += wt * c[0], acc.y += wt * c[1], acc.z += wt * c[2], acc.w += wt;
        ++views;
    }
    reinterpret_cast<float4*>(a.d_sum)[v] = acc;
    a.d_views[v] = views;
}

extern "C" int nfl_mesh_blend(const nfl_mesh_blend_args* a, void* stream) {
    if (!a || a->n_vertices < 0 || a->n_vertices > INT32_MAX) return NFL_EINVAL;
    if (!nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (a->weighting != NFL_BLEND_COS && a->weighting != NFL_BLEND_UNIFORM) return NFL_EINVAL;
    if (!(a->depth_tol >= 0.f) || !(a->min_cos == a->min_cos)) return NFL_EINVAL;
    if (a->weighting == NFL_BLEND_COS && !(a->min_cos >= 0.f)) return NFL_EINVAL;       // a weight is never negative
    if (a->d_center && !(a->reject >= 0.f)) return NFL_EINVAL;
    if (a->n_depth < 0 || a->n_depth > NMC_MAX_WORDS) return NFL_EINVAL;
    if (a->n_vertices == 0) return NFL_OK;
    if (!a->d_vertices || !a->d_normals || !a->d_sum || !a->d_views) return NFL_EINVAL;
    if (ng_misaligned(a->d_vertices, 4) || ng_misaligned(a->d_normals, 4) || ng_misaligned(a->d_sum, 16) ||
        ng_misaligned(a->d_views, 4) || ng_misaligned(a->d_center, 4) || ng_misaligned(a->d_image_weights, 4)) return NFL_EINVAL;
    if (a->count && (!a->d_pixels || ng_bad(a->d_depth, 4))) return NFL_EINVAL;
    if (a->count == 0 && !a->start) return NFL_OK;
    hipLaunchKernelGGL(nfl_mesh_blend_kernel, dim3(nm_grid(a->n_vertices)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
