// Host-side sweep of the plan builder (csrc/nfl_plan.cpp) over every field configuration the ABI accepts or rejects,
// forward and backward plans, built with -fsanitize=address,undefined by tests/test_plan_sanitizer_cpu.py: the plan is
// fixed-size tables (NFL_MAX_RT row tiles, NFL_MAX_CHUNKS chunks) filled by loops over the configuration, which is
// exactly where an out-of-bounds write would hide.  Prints "plans ok <n> rejected <m>".
// The weight-gradient planner (csrc/nfl_wgrad_plan.cpp) is the same kind of code: for every accepted field, with and without
// the transient head, its job list is built and the launch schedule is run over segment counts, CU counts and both stash
// multipliers, and the invariants the kernels rely on are checked.  Prints "wgrad plans <n> schedules <m>" and the rows of the
// instantiation table (WG_INST) that some configuration reaches.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../include/nerf_fl_amd.h"
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

int main() {
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
    return 0;
}
