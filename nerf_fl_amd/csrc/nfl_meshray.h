// nfl_meshray.h -- a camera ray against a triangle: what the two rasters of the geometry layer share (nfl_meshcolor.hip: the
// depth map; nfl_meshrender.hip: the visibility buffer and the shading pass), written ONCE so that both give the same bits.
// include/nerf_fl_amd.h, "mesh colour" and "mesh render"; DESIGN.md sections 25 and 27.  The raster WALK (per-triangle cull
// and box, small-box loop, ballot, wave stride) is not here: as a function shared by both kernels it changed the depth
// raster's instructions, so each unit has its own (section 27).
#pragma once
#include <math.h>

#include "nfl_geom.h"
#include "nfl_macros.h"

#ifndef NMC_SMALL_BOX
#define NMC_SMALL_BOX 64                                    // pixels: boxes above this are walked by the whole wave
#endif
#define NMC_MAX_WORDS (1ll << 38)                           // words of one run (a grid of 2^30 workgroups)

// (a * x + b * y) + c * z, every operation rounded on its own (the unit is built with -ffp-contract=off)
NFL_DEV float nmc_dot(float a, float b, float c, float x, float y, float z) { return (a * x + b * y) + c * z; }

// camera coordinates of the world point p: q = R^T (p - t)
NFL_DEV void nmc_to_camera(const nfl_image_rec& im, const float p[3], float q[3]) {
    const float wx = p[0] - im.c2w[3], wy = p[1] - im.c2w[7], wz = p[2] - im.c2w[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = nmc_dot(im.c2w[c], im.c2w[4 + c], im.c2w[8 + c], wx, wy, wz);
}

NFL_DEV bool nmc_finite(float v) { return v - v == 0.f; }

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

// what every entry point of the two units checks of its run of images
static inline bool nmc_run_ok(const void* table, int32_t n_images, int32_t first, int32_t count) {
    if (!table || reinterpret_cast<uintptr_t>(table) % 8) return false;
    return n_images >= 1 && first >= 0 && count >= 0 && (long long)first + count <= n_images;
}
