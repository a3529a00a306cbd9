// Host-side sweep of the plan builder (csrc/nfl_plan.cpp) over every field configuration the ABI accepts or rejects,
// forward and backward plans, built with -fsanitize=address,undefined by tests/test_plan_sanitizer_cpu.py: the plan is
// fixed-size tables (NFL_MAX_RT row tiles, NFL_MAX_CHUNKS chunks) filled by loops over the configuration, which is
// exactly where an out-of-bounds write would hide.  Prints "plans ok <n> rejected <m>".
// The weight-gradient planner (csrc/nfl_wgrad_plan.cpp) is the same kind of code: for every accepted field, with and without
// the transient head, its job list is built and the launch schedule is run over segment counts, CU counts and both stash
// multipliers, and the invariants the kernels rely on are checked.  Prints "wgrad plans <n> schedules <m>" and the rows of the
// instantiation table (WG_INST) that some configuration reaches.
// The render and dgrad launchers' host side (csrc/nfl_launch.cpp) is the third kind: the ray split over ray, CU and sample
// counts against the twelve lines it replaced; for every accepted field the argument blocks of every mode and backward
// plan, filled over 0x00 and over 0xFF; and the table of refusals of the four entry points.  Prints
// "launch splits <n> fills <m> refusals <k>".
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../include/nerf_fl_amd.h"
#include "../nerf_fl_amd/csrc/nfl_launch.h"
#include "../nerf_fl_amd/csrc/nfl_plan.h"
#include "../nerf_fl_amd/csrc/nfl_wgrad_plan.h"

static bool g_row_reached[WG_N_INST];
#define WG_CHECK(cond)                                                                           \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            printf("wgrad invariant broken: %s (n_seg %d cu %d mult %d)\n", #cond, n_seg, cu, mult); \
            return false;                                                                        \
        }                                                                                        \
    } while (0)

// the job list of an accepted field: table bounds, and every job on a row of the instantiation table
static bool check_wgrad_plan(const WgPlan& P) {
    const int n_seg = -1, cu = -1, mult = -1;
    WG_CHECK(P.n_jobs >= 1 && P.n_jobs <= WG_MAX_JOBS);
    for (int j = 0; j < P.n_jobs; ++j) {
        const WgJob& J = P.job[j];
        WG_CHECK(J.n_ot >= 1 && J.n_ot <= WG_MAX_OT && J.n_it >= 1 && J.n_it <= WG_MAX_IT);
        WG_CHECK(J.n_wo * J.n_wi == 4 && J.n_wo * WG_NOT >= J.n_ot);
        const int nitw = wg_nitw(J.n_it, J.n_wi);
        const int row = wg_inst_row((2 * (J.n_ot + J.n_it) + 3) / 4, nitw);
        WG_CHECK(row >= 0 && P.cost[j] == WG_INST[0][row].cost);
        WG_CHECK(wg_inst_row(P.cost[j], nitw) == row);       // what the schedule and the kernels look up
        g_row_reached[row] = true;
    }
    return true;
}

// one launch schedule of that plan
static bool check_wgrad_schedule(const WgPlan& P, int n_seg, int cu, int mult) {
    WgArgs* A = new WgArgs;              // heap: redzones around the tables
    memset(A, 0, sizeof(*A));
    int n_wg = -1, n_red = -1;
    const int rc = nfl_wgrad_schedule(&P, n_seg, cu, mult, A, &n_wg, &n_red);
    bool ok = [&]() {
        WG_CHECK(rc == NFL_OK);
        const int nj = P.n_jobs, cap = cu < WG_MAX_WGS ? cu : WG_MAX_WGS;
        WG_CHECK(A->n_seg == n_seg && A->wg_start[0] == 0 && A->wg_start[nj] == n_wg);
        // one workgroup per CU -- except that every job needs one of its own: a device with fewer CUs than the plan has jobs
        // gets n_jobs workgroups (some CU runs a second round), which the partial-sum bound below still covers
        WG_CHECK(n_seg < 1 || n_wg <= (cap > nj ? cap : nj));
        long long part_end = 0;
        int red = 0;
        for (int j = 0; j < nj; ++j) {
            const int parts = A->wg_start[j + 1] - A->wg_start[j];
            WG_CHECK(parts >= 0 && parts <= n_seg);
            WG_CHECK(n_seg < 1 || parts >= 1);
            const int row = wg_inst_row(P.cost[j], wg_nitw(P.job[j].n_it, P.job[j].n_wi));
            WG_CHECK(row >= 0 && A->part_nitw[j] == WG_INST[mult - 1][row].nitw && A->part_len[j] == wg_part_len(A->part_nitw[j]));
            WG_CHECK(A->part_off[j] == part_end);           // disjoint: each area starts where the last one ends
            part_end += (long long)parts * A->part_len[j];
            WG_CHECK(A->red_start[j] == red);
            red += 4 * WG_NOT * A->part_nitw[j];
        }
        WG_CHECK(A->red_start[nj] == red && n_red == red);
        WG_CHECK(((long long)NFL_W * NFL_W + part_end) * (long long)sizeof(float) <= (long long)nfl_wgrad_scratch_bytes());
        WG_CHECK(A->slot_bytes > 0 && 2 * A->slot_bytes <= 2 * mult * WG_SLOT);      // the dynamic LDS nfl_mlp_wgrad asks for
        WG_CHECK(A->act_rec == P.act_slots * mult && A->grd_rec == P.grd_slots * mult);
        return true;
    }();
    delete A;
    return ok;
}

// ---------------------------------------------------------------------------------
// csrc/nfl_launch.cpp
// ---------------------------------------------------------------------------------
#define LN_CHECK(cond)                                              \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("launch invariant broken: %s (%s)\n", #cond, ln_where); \
            return false;                                           \
        }                                                           \
    } while (0)
static char ln_where[160];
static int n_splits, n_fills, n_refusals;

static bool check_ray_split() {
    for (int n_rays : {1, 2, 3, 4, 5, 255, 256, 257, 511, 513, 4096, 4097, 1 << 20})
        for (int n_cu : {1, 64, 256, 304})
            for (int n_samples : {1, 31, 32, 33, 64, 96, 128, 129, 256})
                for (int segs_per_tile : {4, 8}) {
                    const int spr = (n_samples + 31) / 32;
                    snprintf(ln_where, sizeof(ln_where), "rays %d cu %d samples %d segs/tile %d", n_rays, n_cu, n_samples, segs_per_tile);
                    int rpw = -1, grid = -1;
                    nfl_ray_split(n_rays, n_cu, segs_per_tile, spr, &rpw, &grid);
                    LN_CHECK(rpw >= 1 && grid == (n_rays + rpw - 1) / rpw && grid >= 1 && grid <= n_cu);
                    LN_CHECK(segs_per_tile / spr <= 1 || rpw % (segs_per_tile / spr) == 0);
                    // the lines both launchers carried before (ncu = n_cu, C::NSLOT or 4 * NCB_ = segs_per_tile, A.spr = spr)
                    const int ncu = n_cu;
                    int rpw0 = (n_rays + ncu - 1) / ncu;
                    const int rays_per_tile = segs_per_tile / spr;
                    if (rays_per_tile > 1) rpw0 = (rpw0 + rays_per_tile - 1) / rays_per_tile * rays_per_tile;
                    if (rpw0 < 1) rpw0 = 1;
                    const int grid0 = (n_rays + rpw0 - 1) / rpw0;
                    LN_CHECK(rpw == rpw0 && grid == grid0);
                    ++n_splits;
                }
    return true;
}

static float g_dev[4];                     // stands for device memory: its address is passed, never followed
static float* const DP = g_dev;
static char* const DC = reinterpret_cast<char*>(g_dev);

static nfl_pass_args pass_args(int n_rays, int n_samples) {
    nfl_pass_args a;
    memset(&a, 0, sizeof(a));
    a.d_rays = DP; a.n_rays = n_rays; a.n_samples = n_samples; a.d_lin = DP; a.d_a_emb = DP;
    return a;
}
static nfl_dgrad_args dgrad_args(int n_rays, int n_samples) {
    nfl_dgrad_args a;
    memset(&a, 0, sizeof(a));
    a.d_head_grads = DP; a.d_act_stash = DC; a.d_grad_stash = DC; a.d_gmax = DP; a.n_rays = n_rays; a.n_samples = n_samples;
    return a;
}

// the fills: every field written from the inputs whatever *out held before
static bool check_render_fill(const NflPlan& P, const nfl_pass_args& a, int mode, float* zc, int zpad) {
    const int n_cu = 256, nslot = 4;
    RenderArgs* A[2] = {new RenderArgs, new RenderArgs};          // heap: redzones
    int grid[2] = {-1, -2};
    for (int i = 0; i < 2; ++i) {
        memset(A[i], i ? 0xFF : 0x00, sizeof(RenderArgs));
        nfl_render_fill(&P, DP, DC, &a, mode, zc, zpad, n_cu, nslot, A[i], &grid[i]);
    }
    const RenderArgs& R = *A[0];
    bool ok = [&]() {
        LN_CHECK(memcmp(A[0], A[1], sizeof(RenderArgs)) == 0 && grid[0] == grid[1]);
        const int use_t = P.has_t && a.d_t_emb && !a.sigma_only;
        LN_CHECK(R.use_t == use_t && R.has_a == P.has_a);
        LN_CHECK(R.n_chunks == (a.sigma_only ? P.n_chunks_sigma : use_t ? P.n_chunks : P.n_chunks_static));
        LN_CHECK(R.n_rt == (a.sigma_only ? P.n_rt_sigma : use_t ? P.n_rt : P.n_rt_static));
        LN_CHECK(R.plan == (const NflPlan*)DP && R.packed == DC && R.bias_off == P.bias_off && R.beta_min == P.beta_min);
        LN_CHECK(R.spr == (a.n_samples + 31) / 32 && R.a.n_rays == a.n_rays && R.a.h_cam == nullptr);
        LN_CHECK(R.nfx_rt == P.n_emb_xyz && R.cx == 6 * P.n_emb_xyz + 3 && R.cd == 6 * R.ndir_rt + 3 && R.n_a == P.n_a && R.n_tau == P.n_tau);
        LN_CHECK(P.ld[NFL_P_DIR] == NFL_W + R.cd + P.n_a);
        LN_CHECK(R.zcache == zc && R.zpad == zpad);
        if (mode == NFL_MODE_EMBED) LN_CHECK(R.n_points == a.n_points && R.emb_stride == a.embedded_stride && !R.gen_rays);
        else LN_CHECK(R.n_points == 0 && R.emb_stride == 0 && R.gen_rays == (a.h_cam || a.d_cam));
        if (mode != NFL_MODE_EMBED && a.h_cam && !a.d_cam) LN_CHECK(memcmp(&R.cam, a.h_cam, sizeof(nfl_camera)) == 0);
        else LN_CHECK(R.cam.width == 0 && R.cam.pix0 == 0 && R.cam.fx == 0.f);
        int rpw = -1, g = -1;
        nfl_ray_split(a.n_rays, n_cu, nslot, R.spr, &rpw, &g);
        LN_CHECK(R.rays_per_wg == rpw && grid[0] == g);
        return true;
    }();
    delete A[0];
    delete A[1];
    ++n_fills;
    return ok;
}

static bool check_render_fills(const NflPlan& P) {
    nfl_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.width = 8; cam.fx = cam.fy = 1.f; cam.pix0 = 5;
    for (int mode : {NFL_MODE_RENDER, NFL_MODE_STASH, NFL_MODE_STASH2, NFL_MODE_EMBED, NFL_MODE_ZCACHE}) {
        const bool x3_only = mode == NFL_MODE_STASH || mode == NFL_MODE_STASH2 || mode == NFL_MODE_ZCACHE;
        if ((x3_only && P.prec != NFL_PREC_F16X3) || (mode == NFL_MODE_ZCACHE && !P.has_a)) continue;      // not admitted
        for (int variant = 0; variant < 3; ++variant) {          // static | transient | sigma only
            if (mode == NFL_MODE_ZCACHE && variant) continue;
            for (int cam_kind = 0; cam_kind < 3; ++cam_kind) {   // ray matrix | host camera | device camera
                if (cam_kind && mode != NFL_MODE_RENDER) continue;
                nfl_pass_args a = pass_args(257, 96);
                a.d_t_emb = variant == 1 ? DP : nullptr;
                a.sigma_only = variant == 2;
                if (cam_kind) { a.d_rays = nullptr; a.h_cam = &cam; }
                if (cam_kind == 2) a.d_cam = reinterpret_cast<const nfl_camera*>(DP);
                if (mode == NFL_MODE_STASH || mode == NFL_MODE_STASH2) { a.d_act_stash = DC; a.stash_split = mode == NFL_MODE_STASH2; }
                if (mode == NFL_MODE_EMBED) nfl_field_forward_args(&P, DP, 1000, 200, variant == 2, variant == 1, DP, &a);
                snprintf(ln_where, sizeof(ln_where), "render fill: prec %d mode %d variant %d camera %d", P.prec, mode, variant, cam_kind);
                LN_CHECK(nfl_render_mode(&P, &a, mode == NFL_MODE_ZCACHE) == mode);
                if (!check_render_fill(P, a, mode, mode == NFL_MODE_ZCACHE ? DP : nullptr, mode == NFL_MODE_ZCACHE ? 128 : 0)) return false;
            }
        }
    }
    return true;
}

static bool check_dgrad_fills(const NflPlan& P, int rays_grad) {
    const int n_cu = 304, ncb = P.prec == NFL_PREC_F16X3 ? 1 : 2;
    for (int ut = 0; ut < 2; ++ut)
        for (int g_rays = 0; g_rays < 2; ++g_rays) {
            snprintf(ln_where, sizeof(ln_where), "dgrad fill: prec %d rays_grad %d use_transient %d d_g_rays %d", P.prec, rays_grad, ut, g_rays);
            nfl_dgrad_args a = dgrad_args(513, 129);
            a.use_transient = ut;
            if (g_rays) { a.d_g_rays = DP; a.d_rays = DP; a.d_z = DP; }
            DgradArgs* A[2] = {new DgradArgs, new DgradArgs};
            int grid[2] = {-1, -2}, rc[2];
            for (int i = 0; i < 2; ++i) {
                memset(A[i], i ? 0xFF : 0x00, sizeof(DgradArgs));
                rc[i] = nfl_dgrad_fill(&P, DP, DC, &a, n_cu, ncb, A[i], &grid[i]);
            }
            const DgradArgs& D = *A[0];
            bool ok = [&]() {
                LN_CHECK(memcmp(A[0], A[1], sizeof(DgradArgs)) == 0 && grid[0] == grid[1] && rc[0] == rc[1]);
                LN_CHECK((P.reserved_flags & 1) == rays_grad && D.rays_tiles == rays_grad && D.ndir_rt == ((P.reserved_flags >> 8) & 0xff));
                LN_CHECK(rc[0] == (g_rays && !rays_grad ? NFL_EINVAL : NFL_OK));
                const int use_t = P.has_t && ut;
                LN_CHECK(D.use_t == use_t && D.has_t == P.has_t && D.has_a == P.has_a && D.n_chunks == P.n_chunks);
                LN_CHECK(D.c_start == (P.has_t && !use_t ? P.n_chunks_sigma : 0));
                LN_CHECK(D.spr == 5 && D.n_seg_total == 513 * 5 && D.nkp == P.nkp && D.nfx_rt == P.n_emb_xyz && D.n_a == P.n_a && D.n_tau == P.n_tau);
                LN_CHECK(D.plan == (const NflPlan*)DP && D.packed == DC && D.a.d_g_rays == a.d_g_rays);
                int rpw = -1, g = -1;
                nfl_ray_split(513, n_cu, 4 * ncb, 5, &rpw, &g);
                if (rc[0] == NFL_OK) LN_CHECK(D.rays_per_wg == rpw && grid[0] == g);
                else LN_CHECK(grid[0] == 0);          // a refused fill leaves nothing to launch
                return true;
            }();
            delete A[0];
            delete A[1];
            ++n_fills;
            if (!ok) return false;
        }
    return true;
}

// One call of a check function: valid arguments for every entry point, until a row's edit.
enum { E_PASS = NFL_ENTRY_PASS, E_FIELD = NFL_ENTRY_FIELD, E_CACHE = NFL_ENTRY_CACHE, E_DGRAD, E_DGRAD_FILL, E_MODE };
enum { ANY, WITH_A, WITHOUT_A };
struct Case {
    const NflPlan *hp, *fx1, *bwd, *bwd_norays;      // hp: the three-product forward plan; the others for the rows that swap it
    NflPlan* edited;                                 // a copy of hp for the rows that damage a plan
    const void *d_plan, *d_packed;
    nfl_pass_args pa;
    const nfl_pass_args* a;
    nfl_camera cam;
    float* zc;
    int n_pad, zmode;
    const float* d_x;
    int n_points, stride, sigma_only, out_t;
    float* d_out;
    nfl_dgrad_args da;
    const nfl_dgrad_args* dga;
};
struct Row {
    int entry, field;
    const char* what;
    void (*edit)(Case&);
    int rc, launch;            // E_MODE: rc = the mode
};
#define BAD NFL_EINVAL
static const Row ROWS[] = {
    // nfl_render_pass
    {E_PASS, WITH_A, "valid", [](Case&) {}, NFL_OK, 1},
    {E_PASS, ANY, "no plan", [](Case& c) { c.hp = nullptr; }, BAD, 0},
    {E_PASS, ANY, "bad magic", [](Case& c) { c.edited->magic = 0; c.hp = c.edited; }, BAD, 0},
    {E_PASS, ANY, "no device plan", [](Case& c) { c.d_plan = nullptr; }, BAD, 0},
    {E_PASS, ANY, "no packed stream", [](Case& c) { c.d_packed = nullptr; }, BAD, 0},
    {E_PASS, ANY, "no arguments", [](Case& c) { c.a = nullptr; }, BAD, 0},
    {E_PASS, ANY, "n_rays < 0", [](Case& c) { c.pa.n_rays = -1; }, BAD, 0},
    {E_PASS, ANY, "n_samples < 1", [](Case& c) { c.pa.n_samples = 0; }, BAD, 0},
    {E_PASS, ANY, "no ray source", [](Case& c) { c.pa.d_rays = nullptr; }, BAD, 0},
    {E_PASS, ANY, "host camera", [](Case& c) { c.pa.d_rays = nullptr; c.pa.h_cam = &c.cam; }, NFL_OK, 1},
    {E_PASS, ANY, "device camera", [](Case& c) { c.pa.d_rays = nullptr; c.pa.d_cam = reinterpret_cast<const nfl_camera*>(DP); }, NFL_OK, 1},
    {E_PASS, ANY, "device camera with a stash", [](Case& c) { c.pa.d_cam = reinterpret_cast<const nfl_camera*>(DP); c.pa.d_act_stash = DC; }, BAD, 0},
    {E_PASS, ANY, "host camera with a stash", [](Case& c) { c.pa.h_cam = &c.cam; c.pa.d_act_stash = DC; }, BAD, 0},
    {E_PASS, ANY, "camera width 0", [](Case& c) { c.cam.width = 0; c.pa.h_cam = &c.cam; }, BAD, 0},
    {E_PASS, ANY, "camera fx 0", [](Case& c) { c.cam.fx = 0.f; c.pa.h_cam = &c.cam; }, BAD, 0},
    {E_PASS, ANY, "camera fy 0", [](Case& c) { c.cam.fy = 0.f; c.pa.h_cam = &c.cam; }, BAD, 0},
    {E_PASS, ANY, "camera pix0 < 0", [](Case& c) { c.cam.pix0 = -1; c.pa.h_cam = &c.cam; }, BAD, 0},
    {E_PASS, ANY, "no depth source", [](Case& c) { c.pa.d_lin = nullptr; }, BAD, 0},
    {E_PASS, ANY, "given depths", [](Case& c) { c.pa.d_lin = nullptr; c.pa.d_z = DP; c.pa.perturb = 1.f; }, NFL_OK, 1},
    {E_PASS, ANY, "jitter without random numbers", [](Case& c) { c.pa.perturb = 1.f; }, BAD, 0},
    {E_PASS, WITH_A, "appearance field without codes", [](Case& c) { c.pa.d_a_emb = nullptr; }, BAD, 0},
    {E_PASS, WITH_A, "... sigma only", [](Case& c) { c.pa.d_a_emb = nullptr; c.pa.sigma_only = 1; }, NFL_OK, 1},
    {E_PASS, WITHOUT_A, "no codes needed", [](Case& c) { c.pa.d_a_emb = nullptr; }, NFL_OK, 1},
    {E_PASS, ANY, "backward plan", [](Case& c) { c.hp = c.bwd; }, BAD, 0},
    {E_PASS, ANY, "fused loss", [](Case& c) { c.pa.d_loss_target = DP; c.pa.d_losses = DP; c.pa.d_seed_rgb = DP; c.pa.loss_slot = 1; }, NFL_OK, 1},
    {E_PASS, ANY, "fused loss without d_losses", [](Case& c) { c.pa.d_loss_target = DP; c.pa.d_seed_rgb = DP; }, BAD, 0},
    {E_PASS, ANY, "fused loss without seeds", [](Case& c) { c.pa.d_loss_target = DP; c.pa.d_losses = DP; }, BAD, 0},
    {E_PASS, ANY, "fused loss slot 2", [](Case& c) { c.pa.d_loss_target = DP; c.pa.d_losses = DP; c.pa.d_seed_rgb = DP; c.pa.loss_slot = 2; }, BAD, 0},
    {E_PASS, ANY, "fused loss slot -1", [](Case& c) { c.pa.d_loss_target = DP; c.pa.d_losses = DP; c.pa.d_seed_rgb = DP; c.pa.loss_slot = -1; }, BAD, 0},
    {E_PASS, ANY, "fused loss, sigma only", [](Case& c) { c.pa.d_loss_target = DP; c.pa.d_losses = DP; c.pa.d_seed_rgb = DP; c.pa.sigma_only = 1; }, BAD, 0},
    {E_PASS, ANY, "fused loss, test extras", [](Case& c) { c.pa.d_loss_target = DP; c.pa.d_losses = DP; c.pa.d_seed_rgb = DP; c.pa.test_extras = 1; }, BAD, 0},
    {E_PASS, ANY, "empty pass", [](Case& c) { c.pa.n_rays = 0; }, NFL_OK, 0},
    {E_PASS, ANY, "empty pass, refused all the same", [](Case& c) { c.pa.n_rays = 0; c.pa.d_lin = nullptr; }, BAD, 0},
    // the kernel mode of a pass (zmode: the cache pass)
    {E_MODE, ANY, "inference", [](Case&) {}, NFL_MODE_RENDER, 0},
    {E_MODE, ANY, "inference, single product", [](Case& c) { c.hp = c.fx1; }, NFL_MODE_RENDER, 0},
    {E_MODE, ANY, "stash", [](Case& c) { c.pa.d_act_stash = DC; }, NFL_MODE_STASH, 0},
    {E_MODE, ANY, "split stash", [](Case& c) { c.pa.d_act_stash = DC; c.pa.stash_split = 1; }, NFL_MODE_STASH2, 0},
    {E_MODE, ANY, "stash, single product", [](Case& c) { c.hp = c.fx1; c.pa.d_act_stash = DC; }, BAD, 0},
    {E_MODE, ANY, "encoded inputs", [](Case& c) { c.pa.d_embedded = DP; c.pa.d_act_stash = DC; }, NFL_MODE_EMBED, 0},
    {E_MODE, ANY, "encoded inputs, single product", [](Case& c) { c.hp = c.fx1; c.pa.d_embedded = DP; }, NFL_MODE_EMBED, 0},
    {E_MODE, ANY, "cache", [](Case& c) { c.zmode = 1; }, NFL_MODE_ZCACHE, 0},
    {E_MODE, ANY, "cache, single product", [](Case& c) { c.hp = c.fx1; c.zmode = 1; }, BAD, 0},
    // nfl_field_forward (stride: set to what the field needs, 0 = compute it)
    {E_FIELD, ANY, "valid", [](Case&) {}, NFL_OK, 1},
    {E_FIELD, ANY, "valid, with the transient columns", [](Case& c) { c.out_t = 1; }, NFL_OK, 1},
    {E_FIELD, ANY, "valid, sigma only", [](Case& c) { c.sigma_only = 1; }, NFL_OK, 1},
    {E_FIELD, ANY, "row one float short", [](Case& c) { c.stride = -1; }, BAD, 0},
    {E_FIELD, ANY, "row one float short, transient", [](Case& c) { c.stride = -1; c.out_t = 1; }, BAD, 0},
    {E_FIELD, ANY, "row one float short, sigma only", [](Case& c) { c.stride = -1; c.sigma_only = 1; }, BAD, 0},
    {E_FIELD, ANY, "no plan", [](Case& c) { c.hp = nullptr; }, BAD, 0},
    {E_FIELD, ANY, "bad magic", [](Case& c) { c.edited->magic = 0; c.hp = c.edited; }, BAD, 0},
    {E_FIELD, ANY, "backward plan", [](Case& c) { c.hp = c.bwd; }, BAD, 0},
    {E_FIELD, ANY, "no device plan", [](Case& c) { c.d_plan = nullptr; }, BAD, 0},
    {E_FIELD, ANY, "no packed stream", [](Case& c) { c.d_packed = nullptr; }, BAD, 0},
    {E_FIELD, ANY, "no input", [](Case& c) { c.d_x = nullptr; }, BAD, 0},
    {E_FIELD, ANY, "no output", [](Case& c) { c.d_out = nullptr; }, BAD, 0},
    {E_FIELD, ANY, "n_points < 0", [](Case& c) { c.n_points = -1; }, BAD, 0},
    {E_FIELD, ANY, "no points", [](Case& c) { c.n_points = 0; }, NFL_OK, 0},
    {E_FIELD, ANY, "no points, refused all the same", [](Case& c) { c.n_points = 0; c.stride = -1; }, BAD, 0},
    // nfl_appearance_cache
    {E_CACHE, WITH_A, "valid", [](Case&) {}, NFL_OK, 1},
    {E_CACHE, WITHOUT_A, "field without appearance", [](Case&) {}, BAD, 0},
    {E_CACHE, WITH_A, "no plan", [](Case& c) { c.hp = nullptr; }, BAD, 0},
    {E_CACHE, WITH_A, "backward plan", [](Case& c) { c.hp = c.bwd; }, BAD, 0},
    {E_CACHE, WITH_A, "no arguments", [](Case& c) { c.a = nullptr; }, BAD, 0},
    {E_CACHE, WITH_A, "no cache", [](Case& c) { c.zc = nullptr; }, BAD, 0},
    {E_CACHE, WITH_A, "single product", [](Case& c) { c.hp = c.fx1; }, BAD, 0},
    {E_CACHE, WITH_A, "n_rays < 0", [](Case& c) { c.pa.n_rays = -1; }, BAD, 0},
    {E_CACHE, WITH_A, "n_samples < 1", [](Case& c) { c.pa.n_samples = 0; }, BAD, 0},
    {E_CACHE, WITH_A, "n_pad < n_samples", [](Case& c) { c.n_pad = 64; }, BAD, 0},
    {E_CACHE, WITH_A, "n_pad no multiple of 64", [](Case& c) { c.n_pad = 100; }, BAD, 0},
    {E_CACHE, WITH_A, "n_pad > 256", [](Case& c) { c.n_pad = 320; }, BAD, 0},
    {E_CACHE, WITH_A, "n_pad 256", [](Case& c) { c.n_pad = 256; }, NFL_OK, 1},
    {E_CACHE, WITH_A, "no ray matrix", [](Case& c) { c.pa.d_rays = nullptr; }, BAD, 0},
    {E_CACHE, WITH_A, "host camera", [](Case& c) { c.pa.h_cam = &c.cam; }, BAD, 0},
    {E_CACHE, WITH_A, "device camera", [](Case& c) { c.pa.d_cam = reinterpret_cast<const nfl_camera*>(DP); }, BAD, 0},
    {E_CACHE, WITH_A, "no codes", [](Case& c) { c.pa.d_a_emb = nullptr; }, BAD, 0},
    {E_CACHE, WITH_A, "transient codes", [](Case& c) { c.pa.d_t_emb = DP; }, BAD, 0},
    {E_CACHE, WITH_A, "sigma only", [](Case& c) { c.pa.sigma_only = 1; }, BAD, 0},
    {E_CACHE, WITH_A, "stash", [](Case& c) { c.pa.d_act_stash = DC; }, BAD, 0},
    {E_CACHE, WITH_A, "fused loss", [](Case& c) { c.pa.d_loss_target = DP; }, BAD, 0},
    {E_CACHE, WITH_A, "encoded inputs", [](Case& c) { c.pa.d_embedded = DP; }, BAD, 0},
    {E_CACHE, WITH_A, "no depth source", [](Case& c) { c.pa.d_lin = nullptr; }, BAD, 0},
    {E_CACHE, WITH_A, "jitter without random numbers", [](Case& c) { c.pa.perturb = 1.f; }, BAD, 0},
    {E_CACHE, WITH_A, "empty pass", [](Case& c) { c.pa.n_rays = 0; }, NFL_OK, 0},
    {E_CACHE, WITH_A, "empty pass, refused all the same", [](Case& c) { c.pa.n_rays = 0; c.n_pad = 100; }, BAD, 0},
    // nfl_mlp_dgrad (hp: the backward plan with ray tiles)
    {E_DGRAD, ANY, "valid", [](Case&) {}, NFL_OK, 1},
    {E_DGRAD, ANY, "no plan", [](Case& c) { c.hp = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "bad magic", [](Case& c) { c.edited->magic = 0; c.hp = c.edited; }, BAD, 0},
    {E_DGRAD, ANY, "forward plan", [](Case& c) { c.hp = c.fx1; }, BAD, 0},
    {E_DGRAD, ANY, "no device plan", [](Case& c) { c.d_plan = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "no packed stream", [](Case& c) { c.d_packed = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "no arguments", [](Case& c) { c.dga = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "no head gradients", [](Case& c) { c.da.d_head_grads = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "no activation stash", [](Case& c) { c.da.d_act_stash = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "no gradient stash", [](Case& c) { c.da.d_grad_stash = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "no gmax", [](Case& c) { c.da.d_gmax = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "n_rays < 0", [](Case& c) { c.da.n_rays = -1; }, BAD, 0},
    {E_DGRAD, ANY, "n_samples < 1", [](Case& c) { c.da.n_samples = 0; }, BAD, 0},
    {E_DGRAD, ANY, "no rays", [](Case& c) { c.da.n_rays = 0; }, NFL_OK, 0},
    {E_DGRAD, ANY, "no rays: returns before the plan's width is looked at", [](Case& c) { c.da.n_rays = 0; c.edited->n_emb_xyz = 0; c.hp = c.edited; }, NFL_OK, 0},
    {E_DGRAD, ANY, "no rays, refused all the same", [](Case& c) { c.da.n_rays = 0; c.da.d_gmax = nullptr; }, BAD, 0},
    {E_DGRAD, ANY, "n_emb_xyz 0", [](Case& c) { c.edited->n_emb_xyz = 0; c.hp = c.edited; }, BAD, 0},
    {E_DGRAD, ANY, "n_emb_xyz 16", [](Case& c) { c.edited->n_emb_xyz = 16; c.hp = c.edited; }, BAD, 0},
    {E_DGRAD, ANY, "ray gradient", [](Case& c) { c.da.d_g_rays = DP; c.da.d_rays = DP; c.da.d_z = DP; }, NFL_OK, 1},
    {E_DGRAD, ANY, "ray gradient from a stream without ray tiles", [](Case& c) { c.hp = c.bwd_norays; c.da.d_g_rays = DP; c.da.d_rays = DP; c.da.d_z = DP; }, BAD, 0},
    {E_DGRAD, ANY, "ray gradient without depths", [](Case& c) { c.da.d_g_rays = DP; c.da.d_rays = DP; }, BAD, 0},
    {E_DGRAD, ANY, "ray gradient without rays", [](Case& c) { c.da.d_g_rays = DP; c.da.d_z = DP; }, BAD, 0},
    {E_DGRAD, ANY, "stream without ray tiles, no ray gradient", [](Case& c) { c.hp = c.bwd_norays; }, NFL_OK, 1},
    // ... and the fill on its own (launch: a grid was computed)
    {E_DGRAD_FILL, ANY, "ray gradient", [](Case& c) { c.da.d_g_rays = DP; c.da.d_rays = DP; c.da.d_z = DP; }, NFL_OK, 1},
    {E_DGRAD_FILL, ANY, "ray gradient from a stream without ray tiles", [](Case& c) { c.hp = c.bwd_norays; c.da.d_g_rays = DP; c.da.d_rays = DP; c.da.d_z = DP; }, BAD, 0},
    {E_DGRAD_FILL, ANY, "ray gradient without depths", [](Case& c) { c.da.d_g_rays = DP; c.da.d_rays = DP; }, BAD, 0},
    {E_DGRAD_FILL, ANY, "ray gradient without rays", [](Case& c) { c.da.d_g_rays = DP; c.da.d_z = DP; }, BAD, 0},
};
#undef BAD

static bool check_refusals(const NflPlan& fx3, const NflPlan& fx1, const NflPlan& bwd, const NflPlan& bwd_norays) {
    Case* c = new Case;
    NflPlan* edited = new NflPlan;
    bool ok = true;
    for (const Row& r : ROWS) {
        if ((r.field == WITH_A && !fx3.has_a) || (r.field == WITHOUT_A && fx3.has_a)) continue;
        const bool dg = r.entry == E_DGRAD || r.entry == E_DGRAD_FILL;
        memset(c, 0, sizeof(*c));
        *edited = dg ? bwd : fx3;
        c->hp = dg ? &bwd : &fx3; c->fx1 = &fx1; c->bwd = &bwd; c->bwd_norays = &bwd_norays; c->edited = edited;
        c->d_plan = DP; c->d_packed = DC;
        c->pa = pass_args(100, 96); c->a = &c->pa;
        c->cam.width = 8; c->cam.fx = c->cam.fy = 1.f;
        c->zc = DP; c->n_pad = 128;
        c->d_x = DP; c->n_points = 1000; c->d_out = DP;
        c->da = dgrad_args(100, 96); c->dga = &c->da;
        r.edit(*c);
        snprintf(ln_where, sizeof(ln_where), "refusals: entry %d, %s", r.entry, r.what);
        int rc = 12345, launch = -1;
        if (r.entry == E_MODE) {
            rc = nfl_render_mode(c->hp, c->a, c->zmode);
            launch = 0;
        } else if (r.entry == E_DGRAD) {
            rc = nfl_dgrad_check(c->hp, c->d_plan, c->d_packed, c->dga, &launch);
        } else if (r.entry == E_DGRAD_FILL) {
            DgradArgs* A = new DgradArgs;
            int grid = -1;
            rc = nfl_dgrad_fill(c->hp, c->d_plan, c->d_packed, c->dga, 256, 2, A, &grid);
            launch = grid > 0;
            delete A;
        } else if (r.entry == E_FIELD) {
            if (c->stride <= 0 && c->hp) {        // exactly the row the field reads (0), or one float less (-1)
                const NflPlan& P = *c->hp;
                const int cx = 6 * P.n_emb_xyz + 3, cd = P.ld[NFL_P_DIR] - NFL_W - P.n_a;
                c->stride += c->sigma_only ? cx : cx + cd + P.n_a + (c->out_t && P.has_t ? P.n_tau : 0);
            }
            nfl_field_forward_args(c->hp, c->d_x, c->n_points, c->stride, c->sigma_only, c->out_t, c->d_out, &c->pa);
            rc = nfl_render_check(r.entry, c->hp, c->d_plan, c->d_packed, &c->pa, nullptr, 0, &launch);
        } else {
            const bool cache = r.entry == E_CACHE;
            rc = nfl_render_check(r.entry, c->hp, c->d_plan, c->d_packed, c->a, cache ? c->zc : nullptr, cache ? c->n_pad : 0, &launch);
        }
        ++n_refusals;
        if (rc != r.rc || launch != r.launch) {
            printf("launch invariant broken: rc %d launch %d, expected %d %d (%s)\n", rc, launch, r.rc, r.launch, ln_where);
            ok = false;
            break;
        }
    }
    delete edited;
    delete c;
    return ok;
}

// everything above for one accepted field
static bool check_launch(const nfl_field_desc& d) {
    NflPlan* p[6];
    for (NflPlan*& q : p) q = new NflPlan;
    bool ok = nfl_plan_fill(&d, NFL_PREC_F16X3, p[0]) == 0 && nfl_plan_fill(&d, NFL_PREC_F16, p[1]) == 0;
    ok = ok && check_render_fills(*p[0]) && check_render_fills(*p[1]);
    for (int bp = 0; ok && bp < 3; ++bp) {
        ok = nfl_plan_fill_bwd(&d, 0, bp, p[2 + bp % 2]) == 0 && nfl_plan_fill_bwd(&d, 1, bp, p[4 + bp % 2]) == 0;
        ok = ok && check_dgrad_fills(*p[2 + bp % 2], 0) && check_dgrad_fills(*p[4 + bp % 2], 1);
    }
    ok = ok && check_refusals(*p[0], *p[1], *p[4], *p[2]);
    for (NflPlan* q : p) delete q;
    return ok;
}

int main() {
    if (!check_ray_split()) return 1;
    int n_ok = 0, n_bad = 0, n_wplans = 0, n_sched = 0;
    for (int xyz = 0; xyz <= 16; ++xyz)
        for (int dir = 0; dir <= 5; ++dir)
            for (int a = 0; a < 2; ++a)
                for (int t = 0; t < 2; ++t)
                    for (int na : {0, 1, 24, 32, 33, 48, 49})
                        for (int nt : {0, 1, 8, 16, 17}) {
                            nfl_field_desc d;
                            memset(&d, 0, sizeof(d));
                            d.n_emb_xyz = xyz; d.n_emb_dir = dir; d.encode_appearance = a; d.n_a = na;
                            d.encode_transient = t; d.n_tau = nt; d.beta_min = 0.1f;
                            NflPlan* p = new NflPlan;          // heap: redzones around the tables
                            for (int prec = 0; prec < 3; ++prec) (nfl_plan_fill(&d, prec, p) == 0 ? n_ok : n_bad)++;
                            for (int rg = 0; rg < 2; ++rg)
                                for (int bp = 0; bp < 4; ++bp) {
                                    const int rc = nfl_plan_fill_bwd(&d, rg, bp, p);
                                    (rc == 0 ? n_ok : n_bad)++;
                                    if (rc == 0 && (p->n_rt > NFL_MAX_RT || p->n_chunks > NFL_MAX_CHUNKS || p->total_ks <= 0)) {
                                        printf("table overflow not rejected: xyz %d dir %d\n", xyz, dir);
                                        return 1;
                                    }
                                }
                            const bool accepted = nfl_plan_fill(&d, NFL_PREC_F16X3, p) == 0;
                            delete p;
                            if (accepted && !check_launch(d)) {
                                printf("  at xyz %d dir %d a %d na %d t %d nt %d\n", xyz, dir, a, na, t, nt);
                                return 1;
                            }
                            for (int ut = 0; ut < 2; ++ut) {
                                WgPlan* w = new WgPlan;
                                const int rc = nfl_wgrad_plan_build(&d, ut, w, nfl_wgrad_plan_bytes());
                                bool ok = (rc == NFL_OK) == accepted;       // no accepted field overflows the job tables
                                if (!ok) printf("wgrad plan: rc %d for an %s field\n", rc, accepted ? "accepted" : "rejected");
                                if (ok && accepted) {
                                    ++n_wplans;
                                    ok = check_wgrad_plan(*w);
                                    for (int mult = 1; ok && mult <= 2; ++mult)
                                        for (int n_seg : {0, 1, 2, 7, 255, 256, 257, 65536, 1048576})
                                            for (int cu : {1, 64, 256, 304}) {
                                                ok = ok && check_wgrad_schedule(*w, n_seg, cu, mult);
                                                ++n_sched;
                                            }
                                }
                                delete w;
                                if (!ok) {
                                    printf("  at xyz %d dir %d a %d na %d t %d nt %d use_transient %d\n", xyz, dir, a, na, t, nt, ut);
                                    return 1;
                                }
                            }
                        }
    printf("plans ok %d rejected %d\n", n_ok, n_bad);
    printf("wgrad plans %d schedules %d\nwgrad rows reached (cost, NITW):", n_wplans, n_sched);
    for (int i = 0; i < WG_N_INST; ++i)
        if (g_row_reached[i]) printf(" (%d, %d)", WG_INST[0][i].cost, WG_INST[0][i].nitw);
    printf("\nwgrad rows not reached:");
    for (int i = 0; i < WG_N_INST; ++i)
        if (!g_row_reached[i]) printf(" (%d, %d)", WG_INST[0][i].cost, WG_INST[0][i].nitw);
    printf("\n");
    printf("launch splits %d fills %d refusals %d\n", n_splits, n_fills, n_refusals);
    return 0;
}
