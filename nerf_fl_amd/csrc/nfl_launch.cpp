// nfl_launch.cpp -- the host side of the render and dgrad launchers (nfl_launch.h).  Plain C++: no runtime call here.
#include "nfl_launch.h"

#include <string.h>

void nfl_ray_split(int n_rays, int n_cu, int segs_per_tile, int spr, int* rays_per_wg, int* grid) {
    int rpw = (n_rays + n_cu - 1) / n_cu;
    const int rays_per_tile = segs_per_tile / spr;
    if (rays_per_tile > 1) rpw = (rpw + rays_per_tile - 1) / rays_per_tile * rays_per_tile;
    if (rpw < 1) rpw = 1;
    *rays_per_wg = rpw;
    *grid = (n_rays + rpw - 1) / rpw;
}

void nfl_field_forward_args(const NflPlan* hp, const float* d_x, int32_t n_points, int32_t row_stride, int32_t sigma_only,
                            int32_t output_transient, float* d_out, nfl_pass_args* a) {
    memset(a, 0, sizeof(*a));
    a->d_embedded = d_x;
    a->n_points = n_points;
    a->embedded_stride = row_stride;
    a->n_rays = n_points > 0 ? (n_points + 31) / 32 : 0;
    a->n_samples = 32;
    a->sigma_only = sigma_only ? 1 : 0;
    a->d_t_emb = (output_transient && hp && hp->has_t && !sigma_only) ? d_x : nullptr;
    a->d_a_emb = a->d_rays = d_x;
    a->d_field_raw = d_out;
}

int nfl_render_check(int entry, const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_pass_args* a,
                     const float* d_zcache, int32_t n_pad, int* launch) {
    *launch = 0;
    // common: a forward plan, the device buffers, a pass of at least one sample per ray
    if (!hp || hp->magic != NFL_PLAN_MAGIC || hp->is_bwd || !d_plan || !d_packed || !a) return NFL_EINVAL;
    if (a->n_rays < 0 || a->n_samples < 1) return NFL_EINVAL;
    if (entry == NFL_ENTRY_FIELD) {         // the encoded matrix: rows wide enough for what the pass reads
        const int cx = 6 * hp->n_emb_xyz + 3, cd = hp->ld[NFL_P_DIR] - NFL_W - hp->n_a;
        const int need = a->sigma_only ? cx : cx + cd + hp->n_a + (a->d_t_emb ? hp->n_tau : 0);
        if (!a->d_embedded || !a->d_field_raw || a->n_points < 0 || a->embedded_stride < need) return NFL_EINVAL;
    } else if (entry == NFL_ENTRY_PASS) {   // a ray source, a camera only for inference, codes, a complete fused loss
        if (!a->d_rays && !a->h_cam && !a->d_cam) return NFL_EINVAL;
        if (a->d_cam && a->d_act_stash) return NFL_EINVAL;
        if (a->h_cam && (a->d_act_stash || a->h_cam->width < 1 || a->h_cam->fx == 0.f || a->h_cam->fy == 0.f || a->h_cam->pix0 < 0))
            return NFL_EINVAL;
        if (!a->sigma_only && hp->has_a && !a->d_a_emb) return NFL_EINVAL;
        if (a->d_loss_target && (!a->d_losses || !a->d_seed_rgb || a->loss_slot < 0 || a->loss_slot > 1 || a->sigma_only ||
                                 a->test_extras)) return NFL_EINVAL;
    } else {                                // the cache: a plain fine pass of a three-product appearance field
        if (!d_zcache || hp->prec != NFL_PREC_F16X3 || !hp->has_a) return NFL_EINVAL;
        if (n_pad < a->n_samples || n_pad % 64 != 0 || n_pad > 64 * NFL_AF_MAXCH) return NFL_EINVAL;
        if (!a->d_rays || a->h_cam || a->d_cam || !a->d_a_emb || a->d_t_emb || a->sigma_only || a->d_act_stash ||
            a->d_loss_target || a->d_embedded) return NFL_EINVAL;
    }
    if (entry != NFL_ENTRY_FIELD) {         // the two that generate depths: given, or linspace (+ the jitter's random numbers)
        if (!a->d_z && !a->d_lin) return NFL_EINVAL;
        if (a->perturb > 0.f && !a->d_z && !a->d_perturb_rand) return NFL_EINVAL;
    }
    *launch = a->n_rays > 0;
    return NFL_OK;
}

int nfl_render_mode(const NflPlan* hp, const nfl_pass_args* a, int zcache) {
    const bool x3 = hp->prec == NFL_PREC_F16X3;
    if (zcache) return x3 ? NFL_MODE_ZCACHE : NFL_EINVAL;
    if (a->d_embedded) return NFL_MODE_EMBED;
    if (!a->d_act_stash) return NFL_MODE_RENDER;
    if (!x3) return NFL_EINVAL;        // the training stash is written by the accurate mode only
    return a->stash_split ? NFL_MODE_STASH2 : NFL_MODE_STASH;
}

void nfl_render_fill(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_pass_args* a, int mode,
                     float* zcache, int zpad, int n_cu, int nslot, RenderArgs* out, int* grid) {
    memset(out, 0, sizeof(*out));
    RenderArgs& A = *out;
    A.plan = static_cast<const NflPlan*>(d_plan);
    A.packed = static_cast<const char*>(d_packed);
    A.a = *a;
    A.a.h_cam = nullptr;                  // a host pointer has no business on the device
    A.has_a = hp->has_a;
    A.use_t = (hp->has_t && a->d_t_emb != nullptr && !a->sigma_only) ? 1 : 0;
    A.n_chunks = a->sigma_only ? hp->n_chunks_sigma : (A.use_t ? hp->n_chunks : hp->n_chunks_static);
    A.n_rt = a->sigma_only ? hp->n_rt_sigma : (A.use_t ? hp->n_rt : hp->n_rt_static);
    A.bias_off = hp->bias_off;
    A.spr = (a->n_samples + 31) / 32;
    A.beta_min = hp->beta_min;
    A.nfx_rt = hp->n_emb_xyz;
    A.ndir_rt = (hp->ld[NFL_P_DIR] - NFL_W - hp->n_a - 3) / 6;
    A.cx = 6 * A.nfx_rt + 3;
    A.cd = 6 * A.ndir_rt + 3;
    A.n_a = hp->n_a;
    A.n_tau = hp->n_tau;
    if (mode == NFL_MODE_EMBED) {      // n_rays = segments of 32 points; d_t_emb != NULL only flags "transient head on"
        A.n_points = a->n_points;
        A.emb_stride = a->embedded_stride;
    } else if (a->h_cam != nullptr || a->d_cam != nullptr) {
        A.gen_rays = 1;
        if (a->d_cam == nullptr) A.cam = *a->h_cam;
    }
    A.zcache = zcache;
    A.zpad = zpad;
    nfl_ray_split(a->n_rays, n_cu, nslot, A.spr, &A.rays_per_wg, grid);
}

// the kernel dereferences d_z and d_rays whenever the stream has ray tiles and d_g_rays is set
static bool dgrad_rays_refused(int rays_tiles, const nfl_dgrad_args* a) {
    return a->d_g_rays && (!rays_tiles || !a->d_rays || !a->d_z);
}

int nfl_dgrad_check(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_dgrad_args* a, int* launch) {
    *launch = 0;
    if (!hp || hp->magic != NFL_PLAN_MAGIC || !hp->is_bwd || !d_plan || !d_packed || !a) return NFL_EINVAL;
    if (!a->d_head_grads || !a->d_act_stash || !a->d_grad_stash || !a->d_gmax) return NFL_EINVAL;
    if (a->n_rays < 0 || a->n_samples < 1) return NFL_EINVAL;
    if (a->n_rays == 0) return NFL_OK;
    if (hp->n_emb_xyz < 1 || hp->n_emb_xyz > NFL_MAX_EMB_XYZ) return NFL_EINVAL;
    if (dgrad_rays_refused(hp->reserved_flags & 1, a)) return NFL_EINVAL;
    *launch = 1;
    return NFL_OK;
}

int nfl_dgrad_fill(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_dgrad_args* a, int n_cu, int ncb,
                   DgradArgs* out, int* grid) {
    memset(out, 0, sizeof(*out));
    *grid = 0;
    DgradArgs& A = *out;
    A.plan = static_cast<const NflPlan*>(d_plan);
    A.packed = static_cast<const char*>(d_packed);
    A.a = *a;
    A.has_a = hp->has_a;
    A.has_t = hp->has_t;
    A.use_t = (hp->has_t && a->use_transient) ? 1 : 0;
    A.n_chunks = hp->n_chunks;
    A.c_start = (hp->has_t && !A.use_t) ? hp->n_chunks_sigma : 0;     // skip the transient head's chunks
    A.spr = (a->n_samples + 31) / 32;
    A.nkp = hp->nkp;
    A.n_seg_total = a->n_rays * A.spr;
    A.rays_tiles = hp->reserved_flags & 1;
    A.nfx_rt = hp->n_emb_xyz;
    A.ndir_rt = (hp->reserved_flags >> 8) & 0xff;
    A.n_a = hp->n_a;
    A.n_tau = hp->n_tau;
    if (dgrad_rays_refused(A.rays_tiles, a)) return NFL_EINVAL;
    nfl_ray_split(a->n_rays, n_cu, 4 * ncb, A.spr, &A.rays_per_wg, grid);
    return NFL_OK;
}
