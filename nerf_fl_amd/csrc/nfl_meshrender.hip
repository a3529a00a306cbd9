// nfl_meshrender.hip -- render a coloured mesh to images (include/nerf_fl_amd.h, "mesh render"): a visibility buffer of the
// mesh per camera (fill + raster) and a shading pass that interpolates vertex attributes at the winning triangle of every
// pixel.  DESIGN.md section 27.
//
// Fill.    A thread per word of the run: 2^64 - 1.
// Raster.  The walk of nfl_mesh_depth's raster (nfl_meshcolor.hip), restated here because sharing it as a function changed
//          that kernel's instructions: a thread per (triangle, image) of the run, the same cull and box (the ray test and
//          the transform ARE shared, nfl_meshray.h), boxes of at most NMC_SMALL_BOX pixels walked by their own lane, larger
//          ones by the whole wave after a ballot (the triangle's number goes round with its coordinates, 15 words).  A hit
//          is a 64-bit atomicMin of (bits(distance) << 32) | triangle: the distance decides, the lower index wins a tie, and
//          the result does not depend on the order of the hits.
// Shade.   A thread per word.  Its image by a binary search of pix0 (as nfl_gather_batch), its pixel from the width, its
//          triangle from the word's low half.  The thread transforms the three vertices and recomputes u, v and the
//          distance with the raster's own expressions (the same bits), interpolates, writes.  The buffer is the caller's:
//          a triangle number or a vertex index out of range makes the pixel uncovered, nothing is read out of range.
#include <math.h>

#include "nfl_geom.h"
#include "nfl_meshray.h"

#define NMR_EMPTY 0xFFFFFFFFFFFFFFFFull

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_visibility_fill_kernel(unsigned long long* vis, i64 n) {
    const i64 w = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (w < n) vis[w] = NMR_EMPTY;
}

NFL_DEV void nmr_pixel(const NmcTri& t, const nfl_image_rec& im, int i, int j, int tr, unsigned long long* vis, i64 base, i64 n_vis) {
    float d;
    if (!nmc_test(t, im, i, j, d)) return;
    if (!(d < __builtin_huge_valf())) return;               // an overflowed distance is no hit: 2^64 - 1 stays "nothing"
    const i64 w = base + (i64)j * im.width + i;
    if (w >= 0 && w < n_vis) atomicMin(vis + w, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)tr);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_visibility_raster_kernel(const nfl_mesh_visibility_args a) {
    const i64 item = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    const i64 T = a.n_triangles, V = a.n_vertices;
    unsigned long long* vis = reinterpret_cast<unsigned long long*>(a.d_vis);
    // every lane stays to the end: the wave's large boxes are walked by all of its lanes
    int n = 0, tri = 0, x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    float q[3][3] = {};
    if (item < T * a.count) {
        n = (int)(item / T);
        const i64 tr = item - (i64)n * T;
        tri = (int)tr;                                      // T <= INT32_MAX / 3
        const int32_t ia = a.d_triangles[3 * tr], ib = a.d_triangles[3 * tr + 1], ic = a.d_triangles[3 * tr + 2];
        const nfl_image_rec& im = a.d_table[a.first + n];
        if (nm_in_range(ia, ib, ic, V) && im.width > 0 && im.height > 0) {
            const int32_t idx[3] = {ia, ib, ic};
            bool finite = true, all_front = true, any_front = false, boxed = true;
            float bx0 = __builtin_huge_valf(), bx1 = -__builtin_huge_valf(), by0 = bx0, by1 = bx1;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float p[3] = {a.d_vertices[3 * (i64)idx[k]], a.d_vertices[3 * (i64)idx[k] + 1], a.d_vertices[3 * (i64)idx[k] + 2]};
                nmc_to_camera(im, p, q[k]);
                finite = finite && nmc_finite(q[k][0]) && nmc_finite(q[k][1]) && nmc_finite(q[k][2]);
                const float s = -q[k][2];
                if (s > 0.f) {
                    any_front = true;
                    const float u = im.cx + im.fx * (q[k][0] / s), v = im.cy - im.fy * (q[k][1] / s);
                    boxed = boxed && nmc_finite(u) && nmc_finite(v);
                    bx0 = fminf(bx0, u), bx1 = fmaxf(bx1, u), by0 = fminf(by0, v), by1 = fmaxf(by1, v);
                } else all_front = false;
            }
            if (finite && any_front) {
                const float wmax = (float)(im.width - 1), hmax = (float)(im.height - 1);
                if (all_front && boxed) {                   // clamped as floats: a projection may lie far outside int range
                    x0 = (int)fminf(fmaxf(floorf(bx0) - 1.f, 0.f), wmax + 1.f), x1 = (int)fmaxf(fminf(ceilf(bx1) + 1.f, wmax), -1.f);
                    y0 = (int)fminf(fmaxf(floorf(by0) - 1.f, 0.f), hmax + 1.f), y1 = (int)fmaxf(fminf(ceilf(by1) + 1.f, hmax), -1.f);
                } else {                                    // straddles the camera plane: no box to trust
                    x0 = 0, x1 = im.width - 1, y0 = 0, y1 = im.height - 1;
                }
            }
        }
    }
    const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    const i64 area = bw > 0 && bh > 0 ? (i64)bw * bh : 0;
    const i64 pix_first = a.d_table[a.first].pix0;
    if (area > 0 && area <= NMC_SMALL_BOX) {
        const nfl_image_rec& im = a.d_table[a.first + n];
        NmcTri t;
        nmc_setup(q[0], q[1], q[2], t);
        const i64 base = im.pix0 - pix_first;
        for (int j = y0; j <= y1; ++j)
            for (int i = x0; i <= x1; ++i) nmr_pixel(t, im, i, j, tri, vis, base, a.n_vis);
    }
    unsigned long long big = __ballot(area > NMC_SMALL_BOX);
    const int lane = threadIdx.x & 63;
    while (big) {
        const int src = __ffsll(big) - 1;
        big &= big - 1;
        float g[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) g[k][c] = __shfl(q[k][c], src);
        const int gn = __shfl(n, src), gx0 = __shfl(x0, src), gy0 = __shfl(y0, src), gw = __shfl(bw, src), gh = __shfl(bh, src);
        const int gtri = __shfl(tri, src);
        const nfl_image_rec& im = a.d_table[a.first + gn];
        NmcTri t;
        nmc_setup(g[0], g[1], g[2], t);
        const i64 base = im.pix0 - pix_first;
        // pixels lane, lane + 64, ... of the box in row-major order, kept as (row, column) and advanced by
        // (64 / gw, 64 % gw) with a carry: no division per pixel
        const int dj = 64 / gw, di = 64 - dj * gw;
        for (int j = lane / gw, i = lane - j * gw; j < gh; j += dj) {
            nmr_pixel(t, im, gx0 + i, gy0 + j, gtri, vis, base, a.n_vis);
            i += di;
            if (i >= gw) i -= gw, ++j;
        }
    }
}

static bool nmr_mesh_ok(const float* ver, const int32_t* tri, i64 V, i64 T) {
    if (!nm_sizes_ok(V, T)) return false;
    if (V && (!ver || reinterpret_cast<uintptr_t>(ver) % 4)) return false;
    return !(T && (!tri || reinterpret_cast<uintptr_t>(tri) % 4));
}

extern "C" int nfl_mesh_visibility(const nfl_mesh_visibility_args* a, void* stream) {
    if (!a || !nmr_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (a->n_vis < 0 || a->n_vis > NMC_MAX_WORDS) return NFL_EINVAL;
    if (a->n_vis && (!a->d_vis || reinterpret_cast<uintptr_t>(a->d_vis) % 8)) return NFL_EINVAL;
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

// (w0 * a + u * b) + v * c
NFL_DEV float nmr_mix(float w0, float u, float v, float a, float b, float c) { return (w0 * a + u * b) + v * c; }

// (uint8)(clamp(c, 0, 1) * 255): truncation; NaN gives 0
NFL_DEV uint8_t nmr_byte(float c) { return (uint8_t)((c > 0.f ? (c < 1.f ? c : 1.f) : 0.f) * 255.f); }

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_shade_kernel(const nfl_mesh_shade_args a) {
    const i64 w = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (w >= a.n_vis) return;
    float rgb[3] = {a.background[0], a.background[1], a.background[2]};
    float depth = __builtin_huge_valf();
    int32_t winner = -1;
    const unsigned long long word = reinterpret_cast<const unsigned long long*>(a.d_vis)[w];
    const i64 tr = (i64)(word & 0xFFFFFFFFull);
    if (word != NMR_EMPTY && tr < a.n_triangles && a.count > 0) {
        // last image of the run whose first word is <= w
        const i64 pix_first = a.d_table[a.first].pix0;
        int lo = a.first, hi = a.first + a.count - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.d_table[mid].pix0 - pix_first <= w) lo = mid; else hi = mid - 1;
        }
        const nfl_image_rec& im = a.d_table[lo];
        const i64 local = w - (im.pix0 - pix_first);
        const int32_t ia = a.d_triangles[3 * tr], ib = a.d_triangles[3 * tr + 1], ic = a.d_triangles[3 * tr + 2];
        if (nm_in_range(ia, ib, ic, a.n_vertices) && im.width > 0 && im.height > 0 && local >= 0 && local < (i64)im.width * im.height) {
            const int j = (int)(local / im.width), i = (int)(local - (i64)j * im.width);
            const int32_t idx[3] = {ia, ib, ic};
            float q[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float p[3] = {a.d_vertices[3 * (i64)idx[k]], a.d_vertices[3 * (i64)idx[k] + 1], a.d_vertices[3 * (i64)idx[k] + 2]};
                nmc_to_camera(im, p, q[k]);
            }
            NmcTri t;
            nmc_setup(q[0], q[1], q[2], t);
            float d, u, v;
            if (nmc_ray<false>(t, im, i, j, d, u, v)) {      // det == 0: no word of the raster's names such a triangle
                const float w0 = (1.f - u) - v;
                depth = d, winner = (int32_t)tr;
                if (a.mode == NFL_SHADE_FACING) {
                    const float dx = ((float)i - im.cx) / im.fx, dy = -((float)j - im.cy) / im.fy, dz = -1.f;
                    const float n0 = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1], n1 = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2],
                                n2 = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
                    float g = fabsf(nmc_dot(n0, n1, n2, dx, dy, dz)) / (sqrtf(nmc_dot(n0, n1, n2, n0, n1, n2)) * sqrtf(nmc_dot(dx, dy, dz, dx, dy, dz)));
                    if (!(g == g)) g = 0.f;
                    rgb[0] = rgb[1] = rgb[2] = g;
                } else {
                    float m[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        m[k] = nmr_mix(w0, u, v, a.d_attr[3 * (i64)ia + k], a.d_attr[3 * (i64)ib + k], a.d_attr[3 * (i64)ic + k]);
                    if (a.mode == NFL_SHADE_NORMAL) {
                        const float len = sqrtf(nmc_dot(m[0], m[1], m[2], m[0], m[1], m[2]));
#pragma unroll
                        for (int k = 0; k < 3; ++k) m[k] = len > 0.f ? 0.5f * (m[k] / len) + 0.5f : 0.5f;      // 0 or NaN: grey
                    }
                    rgb[0] = m[0], rgb[1] = m[1], rgb[2] = m[2];
                }
            }
        }
    }
    if (a.d_rgb) a.d_rgb[3 * w] = rgb[0], a.d_rgb[3 * w + 1] = rgb[1], a.d_rgb[3 * w + 2] = rgb[2];
    if (a.d_rgb_u8) a.d_rgb_u8[3 * w] = nmr_byte(rgb[0]), a.d_rgb_u8[3 * w + 1] = nmr_byte(rgb[1]), a.d_rgb_u8[3 * w + 2] = nmr_byte(rgb[2]);
    if (a.d_depth) a.d_depth[w] = depth;
    if (a.d_triangle) a.d_triangle[w] = winner;
}

extern "C" int nfl_mesh_shade(const nfl_mesh_shade_args* a, void* stream) {
    if (!a || !nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (a->mode != NFL_SHADE_COLOR && a->mode != NFL_SHADE_NORMAL && a->mode != NFL_SHADE_FACING) return NFL_EINVAL;
    if (a->n_vis < 0 || a->n_vis > NMC_MAX_WORDS) return NFL_EINVAL;
    if (!nmr_mesh_ok(a->d_vertices, a->d_triangles, a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (a->mode != NFL_SHADE_FACING && a->n_vertices && !a->d_attr) return NFL_EINVAL;
    if (reinterpret_cast<uintptr_t>(a->d_attr) % 4 || reinterpret_cast<uintptr_t>(a->d_rgb) % 4 ||
        reinterpret_cast<uintptr_t>(a->d_depth) % 4 || reinterpret_cast<uintptr_t>(a->d_triangle) % 4) return NFL_EINVAL;
    if (a->n_vis == 0) return NFL_OK;
    if (!a->d_vis || reinterpret_cast<uintptr_t>(a->d_vis) % 8) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_mesh_shade_kernel, dim3(nm_grid(a->n_vis)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
