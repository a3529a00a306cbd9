// nfl_render_x3.hip -- instantiations of the fused render kernel, 3-product fp16 mode
// (fp32-class accuracy; default).  One 32-sample segment per wave.
#include "nfl_render_impl.h"

// The instantiations for up to 15 frequencies live in their own translation unit (nfl_render_x3w.hip) so that the two
// halves of the library's longest compile run in parallel.
extern "C" int nfl_launch_zcache_x3_wide(const NflPlan*, const void*, const void*, const nfl_pass_args*, float*, int, void*);

// with zcache: the appearance-cache pass (NFL_MODE_ZCACHE; include/nerf_fl_amd.h, nfl_appearance_cache)
extern "C" int nfl_launch_zcache_x3(const NflPlan* hp, const void* d_plan, const void* d_packed,
                                    const nfl_pass_args* args, float* zcache, int zpad, void* stream) {
    if (hp->n_emb_xyz > NFL_MAX_EMB_XYZ) return NFL_EINVAL;
    if (nfl_kernel_nfx(hp->n_emb_xyz) != 10) return nfl_launch_zcache_x3_wide(hp, d_plan, d_packed, args, zcache, zpad, stream);
    return nfl_launch_render<3, 1, 10>(hp, d_plan, d_packed, args, static_cast<hipStream_t>(stream), zcache, zpad);
}

extern "C" int nfl_launch_render_x3(const NflPlan* hp, const void* d_plan, const void* d_packed,
                                    const nfl_pass_args* args, void* stream) {
    return nfl_launch_zcache_x3(hp, d_plan, d_packed, args, nullptr, 0, stream);
}
