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
// The composition through xyz_encoding_final (csrc/nfl_compose.cpp) and the entry half of the weight-gradient pass
// (nfl_wgrad_check, nfl_wgrad_fill) are the fourth: every task list the two builders make, for every distinct shape the
// descriptor sweep yields, is evaluated on exactly-sized heap blocks by a reference interpreter of the kernel's stated
// meaning and compared, exactly (integer data), with the composition's formulas written directly; a table of refusals,
// one and more rows per `return`.  Prints "compose forward cases <n> backward cases <m> refusal rows <k> wgrad fills <l>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../include/nerf_fl_amd.h"
#include "../nerf_fl_amd/csrc/nfl_compose.h"
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

// ---------------------------------------------------------------------------------
// csrc/nfl_compose.cpp and the entry half of csrc/nfl_wgrad_plan.cpp
// ---------------------------------------------------------------------------------
#define CP_CHECK(cond)                                                 \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("compose invariant broken: %s (%s)\n", #cond, cp_where); \
            return false;                                              \
        }                                                              \
    } while (0)
static char cp_where[200];
static int n_cp_fwd, n_cp_bwd, n_cp_refusals, n_wg_fills;
static const float CP_SENTINEL = 12345.f;

// an operand or an output of exactly its size on the heap: one element past it is an ASan report
struct Blk {
    float* p;
    size_t n;
    explicit Blk(size_t n_) : p(new float[n_]), n(n_) {}
    Blk(const Blk& o) : p(new float[o.n]), n(o.n) { memcpy(p, o.p, n * sizeof(float)); }
    Blk& operator=(const Blk&) = delete;
    ~Blk() { delete[] p; }
    Blk& ints(unsigned seed) {          // integers in [-2, 2]: every partial sum is an integer far below 2^24, exact in any order
        for (size_t i = 0; i < n; ++i) {
            seed = seed * 1664525u + 1013904223u;
            p[i] = (float)((int)((seed >> 16) % 5u) - 2);
        }
        return *this;
    }
    Blk& fill(float v) {
        for (size_t i = 0; i < n; ++i) p[i] = v;
        return *this;
    }
    bool same(const Blk& o) const { return n == o.n && memcmp(p, o.p, n * sizeof(float)) == 0; }
};

// The two pieces of arithmetic that form no address of a task are built without the sanitizers and optimised (the sweep
// makes ~4 x 10^10 multiply-adds): the dense product below, whose operands cp_gather has read one by one under the
// sanitizers, and the expected values of the gradient composition.
#define CP_FAST __attribute__((optimize("O3"), no_sanitize("address", "undefined")))
// C (M x N, dense) += A (M x K, dense) B (K x N, dense)
CP_FAST static void cp_dense(float* C, const float* A, const float* B, int M, int N, int K) {
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k) {
            const float a = A[(size_t)m * K + k];
            for (int n = 0; n < N; ++n) C[(size_t)m * N + n] += a * B[(size_t)k * N + n];
        }
}
// rows x cols elements of P at element strides (sr, sc), read one by one, into a dense block
static Blk cp_gather(const float* P, int rows, int cols, long sr, long sc) {
    Blk d((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) d.p[(size_t)r * cols + c] = P[r * sr + c * sc];
    return d;
}

// The reference interpreter: a task list on host memory by the kernel's stated meaning (csrc/nfl_compose.h),
//   C[m*ldc + n] = sum_k A[m*sam + k*sak] B[k*sbk + n*sbn] (+ second product) (+ u[m] v[n]) (+ addm[m]),  m < M, n < N,
// written workgroup by workgroup as tiles_n and tile0 say: workgroup w belongs to the last task whose tile0 is <= w and
// writes the 32 rows from 32 (tile / tiles_n) on, columns 32 (tile % tiles_n) + 0..31 below N.
static bool cp_run(const WgCompose& Cc) {
    CP_CHECK(Cc.n_tasks >= 0 && Cc.n_tasks <= WG_MAX_GEMM);
    int wg = 0;
    for (int ti = 0; ti < Cc.n_tasks; ++ti) {
        const WgGemm& T = Cc.t[ti];
        CP_CHECK(T.tile0 == wg);
        Blk C((size_t)T.M * T.N);
        C.fill(0.f);
        cp_dense(C.p, cp_gather(T.A, T.M, T.K, T.sam, T.sak).p, cp_gather(T.B, T.K, T.N, T.sbk, T.sbn).p, T.M, T.N, T.K);
        if (T.K2) cp_dense(C.p, cp_gather(T.A2, T.M, T.K2, T.sam2, T.sak2).p, cp_gather(T.B2, T.K2, T.N, T.sbk2, T.sbn2).p, T.M, T.N, T.K2);
        const int end = ti + 1 < Cc.n_tasks ? Cc.t[ti + 1].tile0 : Cc.n_wg;
        int written = 0;
        for (; wg < end; ++wg) {
            const int tile = wg - T.tile0, m0 = 32 * (tile / T.tiles_n), n0 = 32 * (tile % T.tiles_n);
            CP_CHECK(m0 + 32 <= T.M);          // the kernel does not test m
            for (int m = m0; m < m0 + 32; ++m)
                for (int n = n0; n < n0 + 32 && n < T.N; ++n, ++written)
                    T.Cp[(size_t)m * T.ldc + n] = C.p[(size_t)m * T.N + n] + (T.u ? T.u[m] * T.v[n] : 0.f) + (T.addm ? T.addm[m] : 0.f);
        }
        CP_CHECK(written == T.M * T.N);        // every element of the block by exactly one workgroup
    }
    CP_CHECK(wg == Cc.n_wg);
    return true;
}

// out[:, :cols] of a (rows x ld) block equals the dense `exp`; every other column still holds what `before` holds
static bool cp_block_is(const Blk& out, const Blk& before, int rows, int ld, int cols, const Blk& exp) {
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < ld; ++c) {
            const size_t i = (size_t)r * ld + c;
            if (c < cols ? out.p[i] != exp.p[(size_t)r * cols + c] : memcmp(&out.p[i], &before.p[i], sizeof(float)) != 0) {
                printf("compose invariant broken: element (%d, %d) is %g (%s)\n", r, c, out.p[i], cp_where);
                return false;
            }
        }
    return true;
}

struct CpShape { int n_side, has_t, n_tau; };      // of a field: side columns of dir_encoding.0, transient layers, their code width

// The forward fold against  W' = [W[:, :256] W_fin | W[:, 256:]],  b' = b + W[:, :256] b_fin.
CP_FAST static void cp_expect_forward(int ld, const float* Wl, const float* bl, const float* Wfin, const float* bfin, float* eW, float* eb) {
    const int W = NFL_W, H = NFL_W / 2;
    for (int r = 0; r < H; ++r) {
        for (int c = 0; c < W; ++c) eW[r * W + c] = 0.f;
        for (int j = 0; j < W; ++j)
            for (int c = 0; c < W; ++c) eW[r * W + c] += Wl[r * ld + j] * Wfin[j * W + c];
        eb[r] = bl[r];
        for (int j = 0; j < W; ++j) eb[r] += Wl[r * ld + j] * bfin[j];
    }
}
static bool check_compose_forward(const CpShape& s) {
    const int W = NFL_W, H = NFL_W / 2, ld[2] = {W + s.n_side, W + s.n_tau};
    snprintf(cp_where, sizeof(cp_where), "forward: n_side %d has_t %d n_tau %d", s.n_side, s.has_t, s.n_tau);
    Blk Wfin((size_t)W * W), bfin(W);
    Wfin.ints(1); bfin.ints(2);
    Blk Wl[2] = {Blk((size_t)H * ld[0]), Blk((size_t)H * ld[1])}, bl[2] = {Blk(H), Blk(H)};
    for (int i = 0; i < 2; ++i) { Wl[i].ints(3 + i); bl[i].ints(5 + i); }
    nfl_field_params P;
    memset(&P, 0, sizeof(P));
    P.weight[NFL_P_FINAL] = Wfin.p; P.bias[NFL_P_FINAL] = bfin.p;
    P.weight[NFL_P_DIR] = Wl[0].p; P.bias[NFL_P_DIR] = bl[0].p;
    P.weight[NFL_P_T0] = Wl[1].p; P.bias[NFL_P_T0] = bl[1].p;
    Blk Wc[2] = {Wl[0], Wl[1]}, bc[2] = {Blk(H), Blk(H)};       // the API takes copies of the weights and writes the biases
    if (!s.has_t) Wc[1].fill(CP_SENTINEL);                      // ... and leaves the transient pair alone without has_t
    bc[0].fill(CP_SENTINEL); bc[1].fill(CP_SENTINEL);
    const Blk Wc0[2] = {Wc[0], Wc[1]}, bc0[2] = {bc[0], bc[1]}, in0[6] = {Wfin, bfin, Wl[0], Wl[1], bl[0], bl[1]};
    WgCompose* Cc = new WgCompose;
    memset(Cc, 0xFF, sizeof(*Cc));
    bool ok = [&]() {
        CP_CHECK(nfl_compose_forward_tasks(&P, s.has_t, s.n_side, s.n_tau, Wc[0].p, bc[0].p, Wc[1].p, bc[1].p, Cc) == NFL_OK);
        CP_CHECK(Cc->n_tasks == (s.has_t ? 4 : 2));
        if (!cp_run(*Cc)) return false;
        for (int i = 0; i < 2; ++i) {
            if (i && !s.has_t) {
                CP_CHECK(Wc[1].same(Wc0[1]) && bc[1].same(bc0[1]));
                continue;
            }
            Blk eW((size_t)H * W), eb(H);
            cp_expect_forward(ld[i], Wl[i].p, bl[i].p, Wfin.p, bfin.p, eW.p, eb.p);
            if (!cp_block_is(Wc[i], Wc0[i], H, ld[i], W, eW) || !cp_block_is(bc[i], bc0[i], H, 1, 1, eb)) return false;
        }
        CP_CHECK(Wfin.same(in0[0]) && bfin.same(in0[1]) && Wl[0].same(in0[2]) && Wl[1].same(in0[3]) && bl[0].same(in0[4]) && bl[1].same(in0[5]));
        return true;
    }();
    delete Cc;
    ++n_cp_fwd;
    return ok;
}

// The gradient composition of one plan and one subset of the four composed gradients (bit 0 dW_fin, 1 db_fin, 2 dW_dir,
// 3 dW_t0) against the formulas of the header of csrc/nfl_wgrad.hip, written directly.
CP_FAST static void cp_expect_backward(int ut, int ld_d, int ld_t, const float* Wfin, const float* bfin, const float* Wdir, const float* Wt0,
                                       const float* G, const float* db_dir, const float* db_t0, float* eWfin, float* ebfin, float* eWdir, float* eWt0) {
    const int W = NFL_W, H = NFL_W / 2;
    // dW_fin = Wd^T G (+ Wt^T Gt),  db_fin = Wd^T db_dir (+ Wt^T db_t0);  Wd = W_dir[:, :256], Gt = rows 128.. of the scratch
    for (int i = 0; i < W; ++i) {
        ebfin[i] = 0.f;
        for (int j = 0; j < W; ++j) eWfin[i * W + j] = 0.f;
    }
    for (int t = 0; t < (ut ? 2 : 1); ++t) {
        const float* Ws = t ? Wt0 : Wdir;
        const float* Gs = G + (size_t)t * H * W;
        const float* dbs = t ? db_t0 : db_dir;
        const int ld = t ? ld_t : ld_d;
        for (int r = 0; r < H; ++r)
            for (int i = 0; i < W; ++i) {
                for (int j = 0; j < W; ++j) eWfin[i * W + j] += Ws[r * ld + i] * Gs[r * W + j];
                ebfin[i] += Ws[r * ld + i] * dbs[r];
            }
    }
    // dW_dir[:, :256] = G W_fin^T + db_dir (x) b_fin, the same for W_t0 from Gt and db_t0
    for (int t = 0; t < 2; ++t) {
        const float* Gs = G + (size_t)t * H * W;
        const float* dbs = t ? db_t0 : db_dir;
        float* e = t ? eWt0 : eWdir;
        for (int r = 0; r < H; ++r)
            for (int i = 0; i < W; ++i) {
                float a = dbs[r] * bfin[i];
                for (int j = 0; j < W; ++j) a += Gs[r * W + j] * Wfin[i * W + j];
                e[r * W + i] = a;
            }
    }
}

static bool check_compose_backward(const WgPlan& P, const CpShape& s, int ut, int subset, const Blk* in, const Blk* in0, const Blk* exp,
                                   const Blk* out0) {
    const int W = NFL_W, H = NFL_W / 2, ld_d = W + s.n_side, ld_t = W + s.n_tau;
    snprintf(cp_where, sizeof(cp_where), "backward: n_side %d has_t %d n_tau %d transient %d subset %d", s.n_side, s.has_t, s.n_tau, ut, subset);
    const Blk &Wfin = in[0], &bfin = in[1], &Wdir = in[2], &Wt0 = in[3], &G = in[4], &db_dir = in[5], &db_t0 = in[6];
    Blk gWfin(out0[0]), gbfin(out0[1]), gWdir(out0[2]), gWt0(out0[3]);        // copies of the sentinel-filled blocks
    nfl_field_params prm;
    nfl_field_grads gr;
    memset(&prm, 0, sizeof(prm));
    memset(&gr, 0, sizeof(gr));
    prm.weight[NFL_P_FINAL] = Wfin.p; prm.bias[NFL_P_FINAL] = bfin.p; prm.weight[NFL_P_DIR] = Wdir.p;
    if (s.has_t) prm.weight[NFL_P_T0] = Wt0.p;
    gr.bias[NFL_P_DIR] = db_dir.p; gr.bias[NFL_P_T0] = db_t0.p;
    if (subset & 1) gr.weight[NFL_P_FINAL] = gWfin.p;
    if (subset & 2) gr.bias[NFL_P_FINAL] = gbfin.p;
    if (subset & 4) gr.weight[NFL_P_DIR] = gWdir.p;
    if (subset & 8) gr.weight[NFL_P_T0] = gWt0.p;
    WgCompose* Cc = new WgCompose;
    memset(Cc, 0xFF, sizeof(*Cc));
    bool ok = [&]() {
        CP_CHECK(nfl_wgrad_check(&P, DP, DC, DC, DP, 64, 64, NFL_PREC_F16, &prm, G.p, &gr) == NFL_OK);
        CP_CHECK(nfl_compose_backward_tasks(&P, &prm, &gr, G.p, Cc) == NFL_OK);
        CP_CHECK(wg_plan_transient(&P) == (ut != 0));
        CP_CHECK(Cc->n_tasks == !!(subset & 1) + !!(subset & 2) + !!(subset & 4) + (ut && (subset & 8)));
        if (!cp_run(*Cc)) return false;
        // a gradient that is not given, or not composed by this plan, keeps its sentinel in every byte
        if (subset & 1 ? !cp_block_is(gWfin, out0[0], W, W, W, exp[0]) : !gWfin.same(out0[0])) return false;
        if (subset & 2 ? !cp_block_is(gbfin, out0[1], W, 1, 1, exp[1]) : !gbfin.same(out0[1])) return false;
        if (subset & 4 ? !cp_block_is(gWdir, out0[2], H, ld_d, W, exp[2]) : !gWdir.same(out0[2])) return false;
        if (ut && (subset & 8) ? !cp_block_is(gWt0, out0[3], H, ld_t, W, exp[3]) : !gWt0.same(out0[3])) return false;
        CP_CHECK(Wfin.same(in0[0]) && bfin.same(in0[1]) && Wdir.same(in0[2]) && Wt0.same(in0[3]) && G.same(in0[4]) && db_dir.same(in0[5]) && db_t0.same(in0[6]));
        return true;
    }();
    delete Cc;
    ++n_cp_bwd;
    return ok;
}

// nfl_wgrad_fill: the zero list whatever *zero held before, the pointer fields of *args and nothing else of it
static bool check_wgrad_fill(const WgPlan& P) {
    snprintf(cp_where, sizeof(cp_where), "nfl_wgrad_fill");
    nfl_field_grads gr;
    memset(&gr, 0, sizeof(gr));
    for (int L = 0; L < NFL_NUM_LAYERS; L += 2) { gr.weight[L] = DP + 1; gr.bias[L] = DP + 2; }
    WgTensors* T[2] = {new WgTensors, new WgTensors};
    WgArgs* A[2] = {new WgArgs, new WgArgs};
    for (int i = 0; i < 2; ++i) {
        memset(T[i], i ? 0xFF : 0x00, sizeof(WgTensors));
        memset(A[i], i ? 0xFF : 0x00, sizeof(WgArgs));
        nfl_wgrad_fill(&P, DP, DC, DC + 1, &gr, DP, A[i], T[i]);
    }
    bool ok = [&]() {
        for (int i = 0; i < 2; ++i) {
            for (int L = 0; L < NFL_NUM_LAYERS; ++L) {
                CP_CHECK(T[i]->ptr[L] == gr.weight[L] && T[i]->n[L] == P.w_numel[L]);
                CP_CHECK(T[i]->ptr[NFL_NUM_LAYERS + L] == gr.bias[L] && T[i]->n[NFL_NUM_LAYERS + L] == P.b_numel[L]);
            }
            CP_CHECK(T[i]->ptr[WG_NTENS - 1] == DP && T[i]->n[WG_NTENS - 1] == NFL_W * NFL_W);
            CP_CHECK(A[i]->plan == (const WgPlan*)DP && A[i]->act == DC && A[i]->grd == DC + 1 && A[i]->scratch == DP);
            CP_CHECK(A[i]->partial == DP + NFL_W * NFL_W && memcmp(&A[i]->g, &gr, sizeof(gr)) == 0);
            CP_CHECK(A[i]->n_seg == (i ? -1 : 0) && A[i]->slot_bytes == (i ? -1 : 0) && A[i]->red_start[WG_MAX_JOBS] == (i ? -1 : 0));
        }
        return true;
    }();
    for (int i = 0; i < 2; ++i) { delete T[i]; delete A[i]; }
    ++n_wg_fills;
    return ok;
}

// One call of nfl_wgrad_check or of a builder: valid arguments, until a row's edit.
enum { C_CHECK, C_FWD, C_BWD };
struct CCase {
    const WgPlan *hp, *plan_t, *plan_not;      // hp: the plan with the transient jobs; plan_not: the same field without
    WgPlan* edited;
    const void* d_wplan;
    const char *act, *grd;
    const float* gmax;
    int n_rays, n_samples, prec;
    nfl_field_params prm;
    const nfl_field_params* params;
    nfl_field_grads gr;
    const nfl_field_grads* grads;
    float* scratch;
    int has_t, n_side, n_tau;
    float *wdir_c, *bdir_c, *wt0_c, *bt0_c;
    WgCompose* out;
};
struct CRow {
    int entry;
    const char* what;
    void (*edit)(CCase&);
    int rc, n_tasks;          // n_tasks: of the builders' list (-1: not looked at)
};
#define BAD NFL_EINVAL
static const CRow CROWS[] = {
    // nfl_wgrad_check, in the order of its refusals
    {C_CHECK, "valid", [](CCase&) {}, NFL_OK, -1},
    {C_CHECK, "no plan", [](CCase& c) { c.hp = nullptr; }, BAD, -1},
    {C_CHECK, "bad magic", [](CCase& c) { c.edited->magic = NFL_PLAN_MAGIC; c.hp = c.edited; }, BAD, -1},
    {C_CHECK, "no device plan", [](CCase& c) { c.d_wplan = nullptr; }, BAD, -1},
    {C_CHECK, "no activation stash", [](CCase& c) { c.act = nullptr; }, BAD, -1},
    {C_CHECK, "no gradient stash", [](CCase& c) { c.grd = nullptr; }, BAD, -1},
    {C_CHECK, "no gmax", [](CCase& c) { c.gmax = nullptr; }, BAD, -1},
    {C_CHECK, "no gradient tensors", [](CCase& c) { c.grads = nullptr; }, BAD, -1},
    {C_CHECK, "no parameters", [](CCase& c) { c.params = nullptr; }, BAD, -1},
    {C_CHECK, "no scratch", [](CCase& c) { c.scratch = nullptr; }, BAD, -1},
    {C_CHECK, "no W_fin", [](CCase& c) { c.prm.weight[NFL_P_FINAL] = nullptr; }, BAD, -1},
    {C_CHECK, "no b_fin", [](CCase& c) { c.prm.bias[NFL_P_FINAL] = nullptr; }, BAD, -1},
    {C_CHECK, "no W_dir", [](CCase& c) { c.prm.weight[NFL_P_DIR] = nullptr; }, BAD, -1},
    {C_CHECK, "transient plan without W_t0", [](CCase& c) { c.prm.weight[NFL_P_T0] = nullptr; }, BAD, -1},
    {C_CHECK, "... which a plan without the transient jobs does not need", [](CCase& c) { c.hp = c.plan_not; c.prm.weight[NFL_P_T0] = nullptr; }, NFL_OK, -1},
    {C_CHECK, "dW_dir without db_dir", [](CCase& c) { c.gr.weight[NFL_P_FINAL] = nullptr; c.gr.bias[NFL_P_DIR] = nullptr; }, BAD, -1},
    {C_CHECK, "dW_fin without db_dir", [](CCase& c) { c.gr.weight[NFL_P_DIR] = nullptr; c.gr.bias[NFL_P_DIR] = nullptr; }, BAD, -1},
    {C_CHECK, "neither, no db_dir", [](CCase& c) { c.gr.weight[NFL_P_DIR] = c.gr.weight[NFL_P_FINAL] = nullptr; c.gr.bias[NFL_P_DIR] = nullptr; }, NFL_OK, -1},
    {C_CHECK, "dW_t0 without db_t0", [](CCase& c) { c.gr.weight[NFL_P_FINAL] = nullptr; c.gr.bias[NFL_P_T0] = nullptr; }, BAD, -1},
    {C_CHECK, "dW_fin without db_t0", [](CCase& c) { c.gr.weight[NFL_P_T0] = nullptr; c.gr.bias[NFL_P_T0] = nullptr; }, BAD, -1},
    {C_CHECK, "... which a plan without the transient jobs does not need", [](CCase& c) { c.hp = c.plan_not; c.gr.bias[NFL_P_T0] = nullptr; }, NFL_OK, -1},
    {C_CHECK, "n_rays < 0", [](CCase& c) { c.n_rays = -1; }, BAD, -1},
    {C_CHECK, "n_samples < 1", [](CCase& c) { c.n_samples = 0; }, BAD, -1},
    {C_CHECK, "no rays", [](CCase& c) { c.n_rays = 0; }, NFL_OK, -1},
    {C_CHECK, "precision 7", [](CCase& c) { c.prec = 7; }, BAD, -1},
    {C_CHECK, "precision -1", [](CCase& c) { c.prec = -1; }, BAD, -1},
    {C_CHECK, "exact-weight chain", [](CCase& c) { c.prec = NFL_PREC_F16W; }, NFL_OK, -1},
    {C_CHECK, "three products", [](CCase& c) { c.prec = NFL_PREC_F16X3; }, NFL_OK, -1},
    {C_CHECK, "scratch off by 4 bytes", [](CCase& c) { c.scratch += 1; }, BAD, -1},
    {C_CHECK, "W_fin off by 4 bytes", [](CCase& c) { c.prm.weight[NFL_P_FINAL] += 1; }, BAD, -1},
    {C_CHECK, "both off by 4 bytes", [](CCase& c) { c.scratch += 1; c.prm.weight[NFL_P_FINAL] += 1; }, BAD, -1},
    {C_CHECK, "scratch off by 8 bytes", [](CCase& c) { c.scratch += 2; }, BAD, -1},
    {C_CHECK, "misaligned, no rays: refused all the same", [](CCase& c) { c.scratch += 1; c.n_rays = 0; }, BAD, -1},
    // nfl_compose_forward_tasks
    {C_FWD, "valid", [](CCase&) {}, NFL_OK, 4},
    {C_FWD, "valid, no transient layers", [](CCase& c) { c.has_t = 0; }, NFL_OK, 2},
    {C_FWD, "... which need neither their outputs nor their parameters", [](CCase& c) { c.has_t = 0; c.wt0_c = c.bt0_c = nullptr; c.prm.weight[NFL_P_T0] = c.prm.bias[NFL_P_T0] = nullptr; }, NFL_OK, 2},
    {C_FWD, "no task list", [](CCase& c) { c.out = nullptr; }, BAD, -1},
    {C_FWD, "no parameters", [](CCase& c) { c.params = nullptr; }, BAD, 0},
    {C_FWD, "no W_dir copy", [](CCase& c) { c.wdir_c = nullptr; }, BAD, 0},
    {C_FWD, "no b_dir output", [](CCase& c) { c.bdir_c = nullptr; }, BAD, 0},
    {C_FWD, "no W_t0 copy", [](CCase& c) { c.wt0_c = nullptr; }, BAD, 0},
    {C_FWD, "no b_t0 output", [](CCase& c) { c.bt0_c = nullptr; }, BAD, 0},
    {C_FWD, "no W_fin", [](CCase& c) { c.prm.weight[NFL_P_FINAL] = nullptr; }, BAD, 0},
    {C_FWD, "no b_fin", [](CCase& c) { c.prm.bias[NFL_P_FINAL] = nullptr; }, BAD, 0},
    {C_FWD, "no W_dir", [](CCase& c) { c.prm.weight[NFL_P_DIR] = nullptr; }, BAD, 0},
    {C_FWD, "no b_dir", [](CCase& c) { c.prm.bias[NFL_P_DIR] = nullptr; }, BAD, 0},
    {C_FWD, "no W_t0", [](CCase& c) { c.prm.weight[NFL_P_T0] = nullptr; }, BAD, 0},
    {C_FWD, "no b_t0", [](CCase& c) { c.prm.bias[NFL_P_T0] = nullptr; }, BAD, 0},
    {C_FWD, "n_side -1", [](CCase& c) { c.n_side = -1; }, BAD, 0},
    {C_FWD, "n_tau -1", [](CCase& c) { c.n_tau = -1; }, BAD, 0},
    {C_FWD, "n_tau -1 without the transient layers", [](CCase& c) { c.has_t = 0; c.n_tau = -1; }, BAD, 0},
    {C_FWD, "no side columns", [](CCase& c) { c.n_side = 0; }, NFL_OK, 4},
    {C_FWD, "misaligned operands: scalar loads", [](CCase& c) { c.prm.weight[NFL_P_FINAL] += 1; c.wdir_c += 1; }, NFL_OK, 4},
    // nfl_compose_backward_tasks
    {C_BWD, "valid", [](CCase&) {}, NFL_OK, 4},
    {C_BWD, "valid, no transient jobs", [](CCase& c) { c.hp = c.plan_not; }, NFL_OK, 3},
    {C_BWD, "no composed gradient wanted", [](CCase& c) { c.gr.weight[NFL_P_FINAL] = c.gr.bias[NFL_P_FINAL] = c.gr.weight[NFL_P_DIR] = c.gr.weight[NFL_P_T0] = nullptr; }, NFL_OK, 0},
    {C_BWD, "no task list", [](CCase& c) { c.out = nullptr; }, BAD, -1},
    {C_BWD, "no plan", [](CCase& c) { c.hp = nullptr; }, BAD, 0},
    {C_BWD, "bad magic", [](CCase& c) { c.edited->magic = NFL_PLAN_MAGIC; c.hp = c.edited; }, BAD, 0},
    {C_BWD, "no parameters", [](CCase& c) { c.params = nullptr; }, BAD, 0},
    {C_BWD, "no gradient tensors", [](CCase& c) { c.grads = nullptr; }, BAD, 0},
    {C_BWD, "no scratch", [](CCase& c) { c.scratch = nullptr; }, BAD, 0},
    {C_BWD, "dW_dir without db_dir", [](CCase& c) { c.gr.bias[NFL_P_DIR] = nullptr; }, BAD, 0},
    {C_BWD, "dW_t0 without db_t0", [](CCase& c) { c.gr.bias[NFL_P_T0] = nullptr; }, BAD, 0},
    {C_BWD, "no W_dir", [](CCase& c) { c.prm.weight[NFL_P_DIR] = nullptr; }, BAD, -1},
    {C_BWD, "no W_t0", [](CCase& c) { c.prm.weight[NFL_P_T0] = nullptr; }, BAD, -1},
    {C_BWD, "no W_fin", [](CCase& c) { c.prm.weight[NFL_P_FINAL] = nullptr; }, BAD, -1},
    {C_BWD, "no b_fin for the rank-1 term", [](CCase& c) { c.prm.bias[NFL_P_FINAL] = nullptr; }, BAD, -1},
    {C_BWD, "db_fin alone without db_dir", [](CCase& c) { c.gr.weight[NFL_P_FINAL] = c.gr.weight[NFL_P_DIR] = c.gr.weight[NFL_P_T0] = nullptr; c.gr.bias[NFL_P_DIR] = nullptr; }, BAD, -1},
    {C_BWD, "scratch off by 4 bytes", [](CCase& c) { c.scratch += 1; }, BAD, -1},
    {C_BWD, "W_fin off by 4 bytes", [](CCase& c) { c.prm.weight[NFL_P_FINAL] += 1; }, BAD, -1},
    {C_BWD, "scratch off by 4 bytes, transient columns only", [](CCase& c) { c.scratch += 1; c.gr.weight[NFL_P_FINAL] = c.gr.bias[NFL_P_FINAL] = c.gr.weight[NFL_P_DIR] = nullptr; }, BAD, -1},
    {C_BWD, "scratch off by 4 bytes, no float4 load of it", [](CCase& c) { c.scratch += 1; c.gr.weight[NFL_P_DIR] = c.gr.weight[NFL_P_T0] = nullptr; }, NFL_OK, 2},
    {C_BWD, "a plan whose W_dir rows are shorter than 256", [](CCase& c) { c.edited->w_numel[NFL_P_DIR] = 128 * 255; c.hp = c.edited; }, BAD, -1},
    {C_BWD, "a plan with more jobs than its table", [](CCase& c) { c.edited->n_jobs = WG_MAX_JOBS + 1; c.hp = c.edited; }, NFL_OK, 3},
};
#undef BAD

alignas(16) static float g_dev16[8];       // made-up device memory again, 16-byte aligned: never followed

static bool check_compose_refusals(const WgPlan& plan_t, const WgPlan& plan_not) {
    CCase* c = new CCase;
    WgPlan* edited = new WgPlan;
    WgCompose* out = new WgCompose;
    float* const D = g_dev16;
    bool ok = true;
    for (const CRow& r : CROWS) {
        memset(c, 0, sizeof(*c));
        memset(out, 0xFF, sizeof(*out));
        *edited = plan_t;
        c->hp = c->plan_t = &plan_t; c->plan_not = &plan_not; c->edited = edited;
        c->d_wplan = D; c->act = c->grd = reinterpret_cast<const char*>(D); c->gmax = D;
        c->n_rays = 64; c->n_samples = 64; c->prec = NFL_PREC_F16;
        for (int L : {NFL_P_FINAL, NFL_P_DIR, NFL_P_T0}) {
            c->prm.weight[L] = c->gr.weight[L] = D;
            c->prm.bias[L] = c->gr.bias[L] = D + 4;
        }
        c->params = &c->prm; c->grads = &c->gr; c->scratch = D;
        c->has_t = 1; c->n_side = 75; c->n_tau = 16;
        c->wdir_c = c->wt0_c = D; c->bdir_c = c->bt0_c = D + 4;
        c->out = out;
        r.edit(*c);
        snprintf(cp_where, sizeof(cp_where), "refusals: entry %d, %s", r.entry, r.what);
        int rc = 12345;
        if (r.entry == C_CHECK)
            rc = nfl_wgrad_check(c->hp, c->d_wplan, c->act, c->grd, c->gmax, c->n_rays, c->n_samples, c->prec, c->params, c->scratch, c->grads);
        else if (r.entry == C_FWD)
            rc = nfl_compose_forward_tasks(c->params, c->has_t, c->n_side, c->n_tau, c->wdir_c, c->bdir_c, c->wt0_c, c->bt0_c, c->out);
        else
            rc = nfl_compose_backward_tasks(c->hp, c->params, c->grads, c->scratch, c->out);
        ++n_cp_refusals;
        if (rc != r.rc || (r.n_tasks >= 0 && out->n_tasks != r.n_tasks) || (rc == NFL_OK && r.entry != C_CHECK && out->n_wg < out->n_tasks)) {
            printf("compose invariant broken: rc %d tasks %d, expected %d %d (%s)\n", rc, out->n_tasks, r.rc, r.n_tasks, cp_where);
            ok = false;
            break;
        }
    }
    delete out;
    delete edited;
    delete c;
    return ok;
}

// the distinct shapes the descriptor sweep yields, each run once: the forward fold per shape, the gradient composition per
// (shape, plan with / without the transient jobs) and subset of the four composed gradients
static CpShape g_cp_fwd_seen[256];
static struct { CpShape s; int ut; } g_cp_bwd_seen[512];
static int n_cp_fwd_seen, n_cp_bwd_seen;
static bool cp_same(const CpShape& a, const CpShape& b) { return a.n_side == b.n_side && a.has_t == b.has_t && a.n_tau == b.n_tau; }

static bool check_compose(const NflPlan& fp, const WgPlan& P) {
    const CpShape s = {fp.ld[NFL_P_DIR] - NFL_W, fp.has_t ? 1 : 0, fp.has_t ? fp.n_tau : 0};
    const int ut = wg_plan_transient(&P) ? 1 : 0;
    snprintf(cp_where, sizeof(cp_where), "shape: n_side %d has_t %d n_tau %d", s.n_side, s.has_t, s.n_tau);
    CP_CHECK(P.w_numel[NFL_P_DIR] == (NFL_W / 2) * (NFL_W + s.n_side) && P.w_numel[NFL_P_T0] == (s.has_t ? (NFL_W / 2) * (NFL_W + s.n_tau) : 0));
    int i = 0;
    while (i < n_cp_fwd_seen && !cp_same(g_cp_fwd_seen[i], s)) ++i;
    if (i == n_cp_fwd_seen) {
        CP_CHECK(n_cp_fwd_seen < 256);
        g_cp_fwd_seen[n_cp_fwd_seen++] = s;
        if (!check_compose_forward(s)) return false;
    }
    i = 0;
    while (i < n_cp_bwd_seen && !(cp_same(g_cp_bwd_seen[i].s, s) && g_cp_bwd_seen[i].ut == ut)) ++i;
    if (i == n_cp_bwd_seen) {
        CP_CHECK(n_cp_bwd_seen < 512);
        g_cp_bwd_seen[n_cp_bwd_seen].s = s;
        g_cp_bwd_seen[n_cp_bwd_seen++].ut = ut;
        // the operands (W_fin, b_fin, W_dir, W_t0, G | Gt, db_dir, db_t0) and the four expected gradients, once for the 16 subsets
        const int W = NFL_W, H = NFL_W / 2, ld_d = W + s.n_side, ld_t = W + s.n_tau;
        Blk in[7] = {Blk((size_t)W * W), Blk(W), Blk((size_t)H * ld_d), Blk((size_t)H * ld_t), Blk((size_t)W * W), Blk(H), Blk(H)};
        for (int k = 0; k < 7; ++k) in[k].ints(11 + k);
        Blk exp[4] = {Blk((size_t)W * W), Blk(W), Blk((size_t)H * W), Blk((size_t)H * W)};
        cp_expect_backward(ut, ld_d, ld_t, in[0].p, in[1].p, in[2].p, in[3].p, in[4].p, in[5].p, in[6].p, exp[0].p, exp[1].p, exp[2].p, exp[3].p);
        const Blk in0[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};          // to see that a run leaves them as they were
        Blk out0[4] = {Blk((size_t)W * W), Blk(W), Blk((size_t)H * ld_d), Blk((size_t)H * ld_t)};       // the outputs' sentinel fill
        for (Blk& b : out0) b.fill(CP_SENTINEL);
        for (int subset = 0; subset < 16; ++subset)
            if (!check_compose_backward(P, s, ut, subset, in, in0, exp, out0)) return false;
    }
    return true;
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
    {   // the refusal table of nfl_wgrad_check and the two compose builders takes no field: once, on the NeRF-W fine field's plans
        nfl_field_desc d;
        memset(&d, 0, sizeof(d));
        d.n_emb_xyz = 10; d.n_emb_dir = 4; d.encode_appearance = 1; d.n_a = 48; d.encode_transient = 1; d.n_tau = 16; d.beta_min = 0.1f;
        WgPlan* w[2] = {new WgPlan, new WgPlan};
        const bool ok = nfl_wgrad_plan_build(&d, 1, w[0], sizeof(WgPlan)) == NFL_OK && nfl_wgrad_plan_build(&d, 0, w[1], sizeof(WgPlan)) == NFL_OK &&
                        check_compose_refusals(*w[0], *w[1]);
        delete w[0];
        delete w[1];
        if (!ok) return 1;
    }
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
                            const NflPlan fp = *p;               // the field's forward plan: the compose shapes are read off it
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
                                    ok = check_wgrad_plan(*w) && check_wgrad_fill(*w) && check_compose(fp, *w);
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
    printf("compose forward cases %d backward cases %d refusal rows %d wgrad fills %d\n", n_cp_fwd, n_cp_bwd, n_cp_refusals, n_wg_fills);
    return 0;
}
