// nfl_meshray.h -- what the mesh image kernels share (nfl_meshcolor.hip: depth map and blend; nfl_meshrender.hip: visibility
// buffer and shading pass; nfl_atlas.hip: the shading pass that samples a texture), each piece written ONCE so that the
// kernels agree bit for bit: the camera transform and the ray test, the raster walk over a sink that takes the hits, the
// shading front (from a visibility word to its pixel, triangle, barycentrics and distance) and its four outputs, the
// interpolation, bilinear and byte rules, and the host checks of a run, a mesh and a buffer of words.
// include/nerf_fl_amd.h, "mesh colour", "mesh render" and "mesh atlas"; DESIGN.md sections 25, 27, 28 and 29.
#pragma once
#include <math.h>

#include "nfl_geom.h"
#include "nfl_macros.h"

#ifndef NMC_SMALL_BOX
#define NMC_SMALL_BOX 64                                    // pixels: boxes above this are walked by the whole wave
#endif
#define NMC_MAX_WORDS (1ll << 38)                           // words of one run (a grid of 2^30 workgroups)
#define NMR_EMPTY 0xFFFFFFFFFFFFFFFFull                     // the visibility word of a pixel that no triangle covers

// (a * x + b * y) + c * z, every operation rounded on its own (the unit is built with -ffp-contract=off)
NFL_DEV float nmc_dot(float a, float b, float c, float x, float y, float z) { return (a * x + b * y) + c * z; }

// camera coordinates of the world point p: q = R^T (p - t)
NFL_DEV void nmc_to_camera(const nfl_image_rec& im, const float p[3], float q[3]) {
    const float wx = p[0] - im.c2w[3], wy = p[1] - im.c2w[7], wz = p[2] - im.c2w[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = nmc_dot(im.c2w[c], im.c2w[4 + c], im.c2w[8 + c], wx, wy, wz);
}

// what a triangle's pixel tests share: the Moeller-Trumbore terms that do not depend on the ray (origin 0: tvec = -a)
struct NmcTri {
    float tv[3], e1[3], e2[3], qv[3], tnum;
};

NFL_DEV void nmc_setup(const float a[3], const float b[3], const float c[3], NmcTri& t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) t.tv[k] = -a[k], t.e1[k] = b[k] - a[k], t.e2[k] = c[k] - a[k];
    t.qv[0] = t.tv[1] * t.e1[2] - t.tv[2] * t.e1[1];
    t.qv[1] = t.tv[2] * t.e1[0] - t.tv[0] * t.e1[2];
    t.qv[2] = t.tv[0] * t.e1[1] - t.tv[1] * t.e1[0];
    t.tnum = nmc_dot(t.e2[0], t.e2[1], t.e2[2], t.qv[0], t.qv[1], t.qv[2]);
}

// The ray of pixel (i, j) against the triangle.  HIT: true, the distance from the camera centre and the barycentrics on a
// hit.  !HIT (the shading pass, for a pixel whose winner is already known): the same expressions without the hit
// conditions, false only when det is 0 or NaN.
template <bool HIT>
NFL_DEV bool nmc_ray(const NmcTri& t, const nfl_image_rec& im, int i, int j, float& depth, float& bu, float& bv) {
    const float dx = ((float)i - im.cx) / im.fx, dy = -((float)j - im.cy) / im.fy, dz = -1.f;
    const float px = dy * t.e2[2] - dz * t.e2[1], py = dz * t.e2[0] - dx * t.e2[2], pz = dx * t.e2[1] - dy * t.e2[0];
    const float det = nmc_dot(t.e1[0], t.e1[1], t.e1[2], px, py, pz);
    if (!(det != 0.f)) return false;                        // 0 or NaN
    const float inv = 1.f / det;
    const float u = nmc_dot(t.tv[0], t.tv[1], t.tv[2], px, py, pz) * inv;
    const float v = nmc_dot(dx, dy, dz, t.qv[0], t.qv[1], t.qv[2]) * inv;
    const float tau = t.tnum * inv;
    if (HIT && !(u >= 0.f && v >= 0.f && u + v <= 1.f && tau > 0.f)) return false;
    depth = tau * sqrtf((dx * dx + dy * dy) + dz * dz);
    bu = u, bv = v;
    return true;
}

// true and the distance from the camera centre on a hit
NFL_DEV bool nmc_test(const NmcTri& t, const nfl_image_rec& im, int i, int j, float& depth) {
    float u, v;
    return nmc_ray<true>(t, im, i, j, depth, u, v);
}

// ---- the raster walk -------------------------------------------------------------------------------------------------------

// pixel (i, j) of image `im`, whose first word in the run is `base`: a hit inside the run's n_words goes to the sink
template <typename Sink>
NFL_DEV void nmc_pixel(const NmcTri& t, const nfl_image_rec& im, int i, int j, int tri, i64 base, i64 n_words, const Sink& sink) {
    float d;
    if (!nmc_test(t, im, i, j, d)) return;
    const i64 w = base + (i64)j * im.width + i;
    if (w >= 0 && w < n_words) sink.hit(d, tri, w);
}

// A thread per (triangle, image) of the run `first .. first + count - 1` of `table`; every thread of the workgroup calls.
// It transforms the three vertices once, culls (all behind the camera plane, a non-finite coordinate, an index out of range)
// and takes a pixel box: the projections' bounding box widened by one pixel and clamped to the frame, or the whole frame
// when the triangle straddles the camera plane.  A box of at most NMC_SMALL_BOX pixels is walked by its own lane.  A larger
// one is NOT: one lane walking thousands of pixels holds its 63 neighbours for as long, so after the small boxes the wave
// ballots its large ones and takes them in turn, all 64 lanes striding the box (the triangle goes round by __shfl).  One
// launch, no list, no second kernel.  A hit on word w of the run is sink.hit(distance, triangle number, w).
template <typename Sink>
NFL_DEV void nmc_raster(const float* ver, const int32_t* tris, i64 V, i64 T, const nfl_image_rec* table, int first, int count,
                        i64 n_words, const Sink& sink) {
    const i64 item = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    // every lane stays to the end: the wave's large boxes are walked by all of its lanes
    int n = 0, tri = 0, x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    float q[3][3] = {};
    if (item < T * count) {
        n = (int)(item / T);
        const i64 tr = item - (i64)n * T;
        tri = (int)tr;                                      // T <= INT32_MAX / 3
        const int32_t ia = tris[3 * tr], ib = tris[3 * tr + 1], ic = tris[3 * tr + 2];
        const nfl_image_rec& im = table[first + n];
        if (nm_in_range(ia, ib, ic, V) && im.width > 0 && im.height > 0) {
            const int32_t idx[3] = {ia, ib, ic};
            bool finite = true, all_front = true, any_front = false, boxed = true;
            float bx0 = __builtin_huge_valf(), bx1 = -__builtin_huge_valf(), by0 = bx0, by1 = bx1;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float p[3] = {ver[3 * (i64)idx[k]], ver[3 * (i64)idx[k] + 1], ver[3 * (i64)idx[k] + 2]};
                nmc_to_camera(im, p, q[k]);
                finite = finite && ng_is_finite(q[k][0]) && ng_is_finite(q[k][1]) && ng_is_finite(q[k][2]);
                const float s = -q[k][2];
                if (s > 0.f) {
                    any_front = true;
                    const float u = im.cx + im.fx * (q[k][0] / s), v = im.cy - im.fy * (q[k][1] / s);
                    boxed = boxed && ng_is_finite(u) && ng_is_finite(v);
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
    const i64 pix_first = table[first].pix0;
    if (area > 0 && area <= NMC_SMALL_BOX) {
        const nfl_image_rec& im = table[first + n];
        NmcTri t;
        nmc_setup(q[0], q[1], q[2], t);
        const i64 base = im.pix0 - pix_first;
        for (int j = y0; j <= y1; ++j)
            for (int i = x0; i <= x1; ++i) nmc_pixel(t, im, i, j, tri, base, n_words, sink);
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
        const nfl_image_rec& im = table[first + gn];
        NmcTri t;
        nmc_setup(g[0], g[1], g[2], t);
        const i64 base = im.pix0 - pix_first;
        // pixels lane, lane + 64, ... of the box in row-major order, kept as (row, column) and advanced by
        // (64 / gw, 64 % gw) with a carry: no division per pixel
        const int dj = 64 / gw, di = 64 - dj * gw;
        for (int j = lane / gw, i = lane - j * gw; j < gh; j += dj) {
            nmc_pixel(t, im, gx0 + i, gy0 + j, gtri, base, n_words, sink);
            i += di;
            if (i >= gw) i -= gw, ++j;
        }
    }
}

// a thread per word of the run: `value`, the word of a pixel that nothing has hit yet
template <typename W>
NFL_DEV void nmc_fill(W* words, i64 n, W value) {
    const i64 w = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (w < n) words[w] = value;
}

// ---- the shading pass ------------------------------------------------------------------------------------------------------

// (w0 * a + u * b) + v * c
NFL_DEV float nmc_mix(float w0, float u, float v, float a, float b, float c) { return (w0 * a + u * b) + v * c; }

// (uint8)(clamp(c, 0, 1) * 255): truncation; NaN gives 0
NFL_DEV uint8_t nmc_byte(float c) { return (uint8_t)((c > 0.f ? (c < 1.f ? c : 1.f) : 0.f) * 255.f); }

// the four taps of a bilinear lookup at the fractions (tx, ty), sx = 1 - tx, sy = 1 - ty: the blend's of an image and the
// shade's of a texture
NFL_DEV float nmc_bilinear(float c00, float c10, float c01, float c11, float sx, float tx, float sy, float ty) {
    return (c00 * sx + c10 * tx) * sy + (c01 * sx + c11 * tx) * ty;
}

// what a covered word of a visibility buffer names: its image and pixel, its triangle with the three indices, and u, v and
// the distance recomputed with the raster's own expressions (the same bits)
struct NmcCovered {
    const nfl_image_rec* im;
    int i, j;
    i64 tr;
    int32_t idx[3];
    NmcTri t;
    float u, v, d;
};

// Word w of the run of `a`, the argument struct of a shading pass: its image by a binary search of pix0 (as
// nfl_gather_batch), its pixel from the width, its triangle from the word's low half.  False for an uncovered word.  The
// buffer is the caller's: a triangle number or a vertex index out of range, or a word past the pixels of its image, makes
// the pixel uncovered, and nothing is read out of range.
template <typename Args>
NFL_DEV bool nmc_covered(const Args& a, i64 w, NmcCovered& c) {
    const unsigned long long word = reinterpret_cast<const unsigned long long*>(a.d_vis)[w];
    c.tr = (i64)(word & 0xFFFFFFFFull);
    if (word == NMR_EMPTY || c.tr >= a.n_triangles || a.count <= 0) return false;
    // last image of the run whose first word is <= w
    const i64 pix_first = a.d_table[a.first].pix0;
    int lo = a.first, hi = a.first + a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.d_table[mid].pix0 - pix_first <= w) lo = mid; else hi = mid - 1;
    }
    const nfl_image_rec& im = a.d_table[lo];
    const i64 local = w - (im.pix0 - pix_first);
    c.im = &im;
#pragma unroll
    for (int k = 0; k < 3; ++k) c.idx[k] = a.d_triangles[3 * c.tr + k];
    if (!nm_in_range(c.idx[0], c.idx[1], c.idx[2], a.n_vertices) || im.width <= 0 || im.height <= 0 || local < 0 ||
        local >= (i64)im.width * im.height) return false;
    c.j = (int)(local / im.width), c.i = (int)(local - (i64)c.j * im.width);
    float q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p[3] = {a.d_vertices[3 * (i64)c.idx[k]], a.d_vertices[3 * (i64)c.idx[k] + 1], a.d_vertices[3 * (i64)c.idx[k] + 2]};
        nmc_to_camera(im, p, q[k]);
    }
    nmc_setup(q[0], q[1], q[2], c.t);
    return nmc_ray<false>(c.t, im, c.i, c.j, c.d, c.u, c.v);     // det == 0: no word of the raster's names such a triangle
}

// the four outputs of a shading pass at word w, each optional
template <typename Args>
NFL_DEV void nmc_shade_out(const Args& a, i64 w, const float rgb[3], float depth, int32_t triangle) {
    if (a.d_rgb) a.d_rgb[3 * w] = rgb[0], a.d_rgb[3 * w + 1] = rgb[1], a.d_rgb[3 * w + 2] = rgb[2];
    if (a.d_rgb_u8) a.d_rgb_u8[3 * w] = nmc_byte(rgb[0]), a.d_rgb_u8[3 * w + 1] = nmc_byte(rgb[1]), a.d_rgb_u8[3 * w + 2] = nmc_byte(rgb[2]);
    if (a.d_depth) a.d_depth[w] = depth;
    if (a.d_triangle) a.d_triangle[w] = triangle;
}

// ---- host: what the entry points check before a launch -----------------------------------------------------------------------

// a run of images of the table
static inline bool nmc_run_ok(const void* table, int32_t n_images, int32_t first, int32_t count) {
    if (ng_bad(table, 8)) return false;
    return n_images >= 1 && first >= 0 && count >= 0 && (long long)first + count <= n_images;
}

// a mesh: sizes in range, and each of the two arrays, where it has any element, present and aligned.  The array of an
// empty side is not looked at; nd_mesh_ok (nfl_geom_layout.h) is the stricter check of the mesh distance and registration calls.
static inline bool nmc_mesh_ok(const float* ver, const int32_t* tri, i64 V, i64 T) {
    if (!nm_sizes_ok(V, T)) return false;
    return !(V && ng_bad(ver, 4)) && !(T && ng_bad(tri, 4));
}

// the n words of a run (depths or visibility): n in range and the buffer, where it has any word, present and aligned
static inline bool nmc_words_ok(const void* words, i64 n, int align) {
    if (n < 0 || n > NMC_MAX_WORDS) return false;
    return !(n && ng_bad(words, align));
}
