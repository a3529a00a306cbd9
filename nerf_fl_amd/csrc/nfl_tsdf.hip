// nfl_tsdf.hip -- fuse depth maps into a truncated signed distance function on a lattice (include/nerf_fl_amd.h, "depth
// fusion"): the accumulation of a run of images, the quotient with its observed flags, and the support of a surface's
// vertices.  DESIGN.md section 32.
//
// Fuse.     A thread per lattice point, the image loop inside (nfl_mesh_blend's pattern): the thread owns its three
//           accumulator words, reads them once and writes them once per run, so there are no atomics and the bits do not
//           depend on how a bank is cut into runs.  The loop variable and the record it names are the same for the whole wave:
//           the record is read through scalar loads, an image weight of 0 is a scalar branch, and a wave none of whose 64
//           points falls into an image's frame skips that image's body in one branch on the execution mask.  Per
//           contributing image one depth word (and one weight word) is gathered, and THAT is what the dealing of points to
//           threads is chosen for: a workgroup is a tile of 16 x 4 x 4 points and a wave 16 x 4 of one plane, which reads
//           and writes its accumulators in 128-byte pieces of four x-rows and projects into a patch of an image a few cache
//           lines large.  A wave of 64 points of ONE x-row projects onto a line as long as 64 cache lines when the row runs
//           down an image: 2.0 x the time with depth words alone and 5.2 x with pixel weights beside them (DESIGN.md
//           section 32).
// Resolve.  A thread per lattice point.
// Support.  A thread per vertex, eight bytes of the flags each.
#include <math.h>

#include "nfl_geom.h"
#include "nfl_meshray.h"

// the points of a workgroup: a tile of NTS_TILE_X x NTS_TILE_Y x NTS_TILE_Z, x fastest over the threads, so a wave is
// NTS_TILE_X x (64 / NTS_TILE_X) points of one plane
#ifndef NTS_TILE_X
#define NTS_TILE_X 16
#define NTS_TILE_Y 4
#endif
#define NTS_TILE_Z (NM_THREADS / (NTS_TILE_X * NTS_TILE_Y))
static_assert(NTS_TILE_X * NTS_TILE_Y * NTS_TILE_Z == NM_THREADS, "a tile is a workgroup");

static inline i64 nts_tiles(int nx, int ny, int nz) {
    return ng_cdiv(nx, NTS_TILE_X) * ng_cdiv(ny, NTS_TILE_Y) * ng_cdiv(nz, NTS_TILE_Z);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_tsdf_fuse_kernel(const nfl_tsdf_fuse_args a) {
    const int tx = (a.nx + NTS_TILE_X - 1) / NTS_TILE_X, ty = (a.ny + NTS_TILE_Y - 1) / NTS_TILE_Y;
    const int bz = blockIdx.x / (tx * ty), rest = blockIdx.x - bz * (tx * ty), by = rest / tx, bx = rest - by * tx;
    const int t = threadIdx.x;
    const int ix0 = bx * NTS_TILE_X + t % NTS_TILE_X, iy0 = by * NTS_TILE_Y + t / NTS_TILE_X % NTS_TILE_Y;
    const int iz0 = bz * NTS_TILE_Z + t / (NTS_TILE_X * NTS_TILE_Y);
    if (ix0 >= a.nx || iy0 >= a.ny || iz0 >= a.nz) return;
    const i64 at = ((i64)iz0 * a.ny + iy0) * a.nx + ix0;
    const float p[3] = {a.lo[0] + (float)ix0 * a.spacing[0], a.lo[1] + (float)iy0 * a.spacing[1], a.lo[2] + (float)iz0 * a.spacing[2]};
    float2 acc = make_float2(0.f, 0.f);
    int32_t views = 0;
    if (!a.start) acc = reinterpret_cast<const float2*>(a.d_acc)[at], views = a.d_views[at];
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
        const float u = im.cx + im.fx * (q[0] / s), v = im.cy - im.fy * (q[1] / s);
        if (!(u >= 0.f && u <= wmax && v >= 0.f && v <= hmax)) continue;                // 3
        const int ix = (int)floorf(u + 0.5f), iy = (int)floorf(v + 0.5f);
        const i64 word = (im.pix0 - pix_first) + (i64)iy * im.width + ix;
        if (word < 0 || word >= a.n_depth) continue;                    // a depth buffer that is not this run's: nothing read
        const float D = a.d_depth[word];
        const float w = wi * (a.d_pixel_weights ? a.d_pixel_weights[word] : 1.f);
        if (!(w > 0.f && D > 0.f)) continue;                                            // 4
        const float ex = im.c2w[3] - p[0], ey = im.c2w[7] - p[1], ez = im.c2w[11] - p[2];
        const float dist = sqrtf((ex * ex + ey * ey) + ez * ez);
        float phi = (dist - D) / a.trunc;
        if (phi > 1.f) continue;                                                        // 5: hidden behind the surface
        phi = fmaxf(phi, -1.f);
        acc.x += w * phi, acc.y += w;
        ++views;
    }
    reinterpret_cast<float2*>(a.d_acc)[at] = acc;
    a.d_views[at] = views;
}

extern "C" int nfl_tsdf_fuse(const nfl_tsdf_fuse_args* a, void* stream) {
    if (!a || !nmc_run_ok(a->d_table, a->n_images, a->first, a->count)) return NFL_EINVAL;
    if (!ng_dims_ok(a->nx, a->ny, a->nz)) return NFL_EINVAL;
    if (!(a->trunc > 0.f)) return NFL_EINVAL;                                           // NaN included
    if (!nmc_words_ok(a->d_depth, a->n_depth, 4)) return NFL_EINVAL;
    if (ng_misaligned(a->d_pixel_weights, 4) || ng_misaligned(a->d_image_weights, 4)) return NFL_EINVAL;
    if (ng_bad(a->d_acc, 8) || ng_bad(a->d_views, 4)) return NFL_EINVAL;
    if (a->count == 0 && !a->start) return NFL_OK;
    const i64 tiles = nts_tiles(a->nx, a->ny, a->nz);                                   // 2^30 points: far below 2^31 tiles
    if (tiles > INT32_MAX) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_tsdf_fuse_kernel, dim3((unsigned)tiles), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NM_THREADS) void nfl_tsdf_resolve_kernel(const nfl_tsdf_resolve_args a) {
    const i64 n_points = (i64)a.nx * a.ny * a.nz;
    const i64 at = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (at >= n_points) return;
    const float2 acc = reinterpret_cast<const float2*>(a.d_acc)[at];
    const bool known = acc.y >= a.min_weight && a.d_views[at] >= a.min_views;
    a.d_lattice[at] = known ? acc.x / acc.y : a.fill;
    a.d_known[at] = known ? 1 : 0;
}

extern "C" int nfl_tsdf_resolve(const nfl_tsdf_resolve_args* a, void* stream) {
    if (!a || !ng_dims_ok(a->nx, a->ny, a->nz)) return NFL_EINVAL;
    if (!(a->min_weight > 0.f) || a->min_views < 1 || !(a->fill == a->fill)) return NFL_EINVAL;
    if (!a->d_acc || !a->d_views || !a->d_lattice || !a->d_known) return NFL_EINVAL;
    if (ng_misaligned(a->d_acc, 8) || ng_misaligned(a->d_views, 4) || ng_misaligned(a->d_lattice, 4)) return NFL_EINVAL;
    const i64 n_points = (i64)a->nx * a->ny * a->nz;
    hipLaunchKernelGGL(nfl_tsdf_resolve_kernel, dim3(nm_grid(n_points)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---- support ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NM_THREADS) void nfl_tsdf_support_kernel(const nfl_tsdf_support_args a) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= a.n_vertices) return;
    const int dims[3] = {a.nx, a.ny, a.nz};
    int lo[3], hi[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float g = (a.d_vertices[3 * v + k] - a.lo[k]) / a.spacing[k];
        inside = inside && ng_is_finite(g) && g >= 0.f && g <= (float)(dims[k] - 1);
        lo[k] = inside ? (int)floorf(g) : 0, hi[k] = inside ? (int)ceilf(g) : 0;
    }
    bool all = inside;
    if (inside) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int x = c & 1 ? hi[0] : lo[0], y = c & 2 ? hi[1] : lo[1], z = c & 4 ? hi[2] : lo[2];
            all = all && a.d_known[((i64)z * a.ny + y) * a.nx + x] != 0;
        }
    }
    a.d_support[v] = all ? 1 : 0;
}

extern "C" int nfl_tsdf_support(const nfl_tsdf_support_args* a, void* stream) {
    if (!a || !ng_dims_ok(a->nx, a->ny, a->nz)) return NFL_EINVAL;
    if (a->n_vertices < 0 || a->n_vertices > INT32_MAX) return NFL_EINVAL;
    if (!a->d_known) return NFL_EINVAL;
    if (a->n_vertices == 0) return NFL_OK;
    if (!a->d_vertices || !a->d_support || ng_misaligned(a->d_vertices, 4)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_tsdf_support_kernel, dim3(nm_grid(a->n_vertices)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
