// nfl_launch.h -- what a launcher of the render and dgrad kernels decides on the host, in plain C++ (nfl_launch.cpp): the
// entry points' argument checks, the kernel mode of a pass, the kernels' argument blocks and their fill, the ray split.
// g++ builds it (tests/plan_sweep.cpp, under the sanitizers); the .hip units pick the instantiation and launch (nfl_dev.h).
#pragma once
#include <stddef.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_plan.h"

#define NFL_MODE_RENDER 0
#define NFL_MODE_STASH 1      // render + fp16 activation stash for the backward
#define NFL_MODE_STASH2 3     // as STASH, with split (hi + lo) activation records for the three-product backward
#define NFL_MODE_EMBED 2      // NeRF.forward on already-encoded inputs (reference models/nerf.py:153-212): no
                              // depth generation / encoding / compositing, 32 points per segment
#define NFL_MODE_ZCACHE 4     // render + the pre-activation of dir_encoding.0 to the appearance cache (nfl_appearance_cache)
#define NFL_AF_MAXCH 4        // ... which holds n_pad <= 256 samples per ray: 4 chunks of 64

// The kernels take the two blocks by value and re-read them from the kernarg segment (nfl_dev.h: nfl_kernarg): a field
// that moves changes every kernel's scalar loads, hence the layout assertions.
struct RenderArgs {
    const NflPlan* plan;      // device copy of the plan
    const char* packed;       // fragment stream, then bias table at plan->bias_off
    nfl_pass_args a;
    int n_chunks;             // chunks per tile consumed by this pass (prefix of the stream)
    int n_rt;                 // row tiles consumed by this pass
    int bias_off;
    int has_a;                // field has the appearance input
    int use_t;                // transient head evaluated in this pass
    int spr;                  // 32-sample segments per ray
    int rays_per_wg;
    float beta_min;
    int n_points, emb_stride;   // NFL_MODE_EMBED: rows / row stride (floats) of a.d_embedded
    int nfx_rt, ndir_rt;        // the field's frequency counts (<= the instantiation's: nfl_plan.h, "Encoder widths")
    int cx, cd;                 // 6 nfx_rt + 3, 6 ndir_rt + 3: widths of the encoded position / direction
    int n_a, n_tau;             // widths of the appearance / transient codes (<= 48 / 16; narrower: the k-steps are zero-padded)
    int gen_rays;               // rays come from `cam` (nfl_pass_args::h_cam), not from a.d_rays
    nfl_camera cam;
    float* zcache;              // NFL_MODE_ZCACHE: the appearance cache (nfl_appearance_cache), else null
    int zpad;                   // its padded sample count
};
static_assert(sizeof(RenderArgs) == 520 && offsetof(RenderArgs, a) == 16 && offsetof(RenderArgs, rays_per_wg) == 368 &&
              offsetof(RenderArgs, zpad) == 512, "the render kernels' kernarg layout");
struct DgradArgs {
    const NflPlan* plan;
    const char* packed;
    nfl_dgrad_args a;
    int n_chunks, c_start;
    int has_a, has_t, use_t;
    int spr, rays_per_wg, nkp, n_seg_total;
    int rays_tiles;           // the stream carries the encoded-position / direction rows (gradient w.r.t. rays)
    int nfx_rt, ndir_rt;      // the field's frequency counts (<= the instantiation's; nfl_plan.h, "Encoder widths")
    int n_a, n_tau;           // widths of the latent codes (<= 48 / 16)
};
static_assert(sizeof(DgradArgs) == 192 && offsetof(DgradArgs, a) == 16 && offsetof(DgradArgs, rays_per_wg) == 160 &&
              offsetof(DgradArgs, n_tau) == 188, "the dgrad kernels' kernarg layout");

// Contiguous ray ranges, one workgroup per CU where there is enough work; whole tiles per workgroup where a tile
// (segs_per_tile 32-sample segments: NflRenderCfg::NSLOT, 4 NCB of the dgrad kernel) holds more than one ray of spr segments.
void nfl_ray_split(int n_rays, int n_cu, int segs_per_tile, int spr, int* rays_per_wg, int* grid);

// The render family.  nfl_render_check: the argument checks of one entry point (d_zcache, n_pad: the cache's only);
// NFL_OK or NFL_EINVAL, and *launch = 0 with NFL_OK for an empty pass.  nfl_field_forward_args: the pass nfl_field_forward
// runs (n_rays = segments of 32 points; d_t_emb / d_a_emb / d_rays only flag what is on).  nfl_render_mode: NFL_MODE_* of a
// checked pass, or NFL_EINVAL (the stash and the cache are written by the three-product kernels only).  nfl_render_fill:
// the argument block and the grid; nslot = NflRenderCfg::NSLOT of the instantiation that runs the mode.
enum { NFL_ENTRY_PASS, NFL_ENTRY_FIELD, NFL_ENTRY_CACHE };       // nfl_render_pass, nfl_field_forward, nfl_appearance_cache
int nfl_render_check(int entry, const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_pass_args* a,
                     const float* d_zcache, int32_t n_pad, int* launch);
void nfl_field_forward_args(const NflPlan* hp, const float* d_x, int32_t n_points, int32_t row_stride, int32_t sigma_only,
                            int32_t output_transient, float* d_out, nfl_pass_args* a);
int nfl_render_mode(const NflPlan* hp, const nfl_pass_args* a, int zcache);
void nfl_render_fill(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_pass_args* a, int mode,
                     float* zcache, int zpad, int n_cu, int nslot, RenderArgs* out, int* grid);
// nfl_mlp_dgrad: its checks, and its argument block and grid (ncb = NflDgradCfg::NCB).  Both refuse (NFL_EINVAL) d_g_rays
// on a stream without ray tiles or without the rays and depths the kernel then reads: the check before the launcher's
// first runtime call, the fill because it is what knows rays_tiles.
int nfl_dgrad_check(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_dgrad_args* a, int* launch);
int nfl_dgrad_fill(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_dgrad_args* a, int n_cu, int ncb,
                   DgradArgs* out, int* grid);
