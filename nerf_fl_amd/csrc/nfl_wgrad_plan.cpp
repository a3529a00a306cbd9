// nfl_wgrad_plan.cpp -- host planner of the weight-gradient pass: the per-layer job list of a field and the launch schedule
// of a call, the entry point's refusals and the fill of its pointer arguments.  Plain C++ (no HIP), so that
// tests/plan_sweep.cpp can run it under ASan + UBSan over every configuration: fixed-size tables (WG_MAX_JOBS, WG_MAX_OT,
// WG_MAX_IT) filled by configuration-dependent loops.
#include "nfl_wgrad_plan.h"

#include <string.h>

// appends the tiles of `count` features; false (nothing more written) when the table of `cap` tiles is full
static bool add_tiles(WgTile* dst, int32_t& n, int cap, int slot0, int kind, int idx0, int count) {
    for (int t = 0; 32 * t < count; ++t) {
        if (n >= cap) return false;
        WgTile w;
        w.slot = (int16_t)(slot0 + 2 * t);
        w.kind = (int16_t)kind;
        w.idx0 = (int16_t)(idx0 + 32 * t);
        w.nvalid = (int16_t)(count - 32 * t < 32 ? count - 32 * t : 32);
        dst[n++] = w;
    }
    return true;
}
static WgJob make_job(int layer, int ld, bool bias) {
    WgJob j;
    memset(&j, 0, sizeof(j));
    j.layer = layer;
    j.ld = ld;
    j.do_bias = bias ? 1 : 0;
    for (int i = 0; i < WG_MAX_OT; ++i) j.bias_layer_of_ot[i] = -1;
    return j;
}
static void finish_job(WgJob& j) {
    if (j.n_ot > 4) { j.n_wo = 4; j.n_wi = 1; }          // 2 out tiles per wave, all in tiles
    else if (j.n_ot > 2) { j.n_wo = 2; j.n_wi = 2; }
    else { j.n_wo = 1; j.n_wi = 4; }                     // heads: split the in tiles
}

extern "C" size_t nfl_wgrad_plan_bytes(void) { return sizeof(WgPlan); }

extern "C" int nfl_wgrad_plan_build(const nfl_field_desc* d, int32_t use_transient, void* h_plan, size_t bytes) {
    NflPlan p;
    if (!d || !h_plan) return NFL_EINVAL;
    if (bytes < sizeof(WgPlan)) return NFL_ESMALL;
    if (nfl_plan_fill(d, NFL_PREC_F16X3, &p) != NFL_OK) return NFL_EINVAL;
    const int nkp = p.nkp, cx = 6 * d->n_emb_xyz + 3, cd = 6 * d->n_emb_dir + 3, W = NFL_W, H = NFL_W / 2;
    const bool ut = p.has_t && use_transient;
    WgPlan& P = *static_cast<WgPlan*>(h_plan);
    memset(&P, 0, sizeof(P));
    P.magic = WG_PLAN_MAGIC;
    P.act_slots = nfl_act_slots(nkp);
    P.grd_slots = NFL_GRD_SLOTS;
    int nj = 0;
    bool ok = true;      // cleared by a job that does not fit the tables or has no instantiation: NFL_EINVAL at the end
    auto out = [&](WgJob& j, int slot0, int kind, int idx0, int count) { ok = ok && add_tiles(j.ot, j.n_ot, WG_MAX_OT, slot0, kind, idx0, count); };
    auto in = [&](WgJob& j, int slot0, int kind, int idx0, int count) { ok = ok && add_tiles(j.it, j.n_it, WG_MAX_IT, slot0, kind, idx0, count); };
    auto push = [&](WgJob j) {
        finish_job(j);
        const int row = wg_inst_row((2 * (j.n_ot + j.n_it) + 3) / 4, wg_nitw(j.n_it, j.n_wi));
        ok = ok && nj < WG_MAX_JOBS && j.n_ot >= 1 && j.n_it >= 1 && row >= 0;
        if (!ok) return;
        P.cost[nj] = WG_INST[0][row].cost;
        P.job[nj++] = j;
    };
    for (int l = 1; l <= 8; ++l) {
        WgJob j = make_job(NFL_P_XYZ1 + l - 1, p.ld[NFL_P_XYZ1 + l - 1], true);
        out(j, NFL_GRD_D(l), NFL_SEG_ACT, 0, W);
        if (l == 1 || l == 5) {
            in(j, 0, NFL_SEG_NAT, 0, cx);
            if (l == 5) {
                push(j);
                j = make_job(NFL_P_XYZ1 + 4, p.ld[NFL_P_XYZ1 + 4], false);
                out(j, NFL_GRD_D(5), NFL_SEG_ACT, 0, W);
                in(j, nfl_act_h(nkp, 4), NFL_SEG_ACT, cx, W);
            }
        } else {
            in(j, nfl_act_h(nkp, l - 1), NFL_SEG_ACT, 0, W);
        }
        push(j);
    }
    if (ut) {   // sigma head (without the transient head it shares the h8 stream of the next job)
        WgJob j = make_job(NFL_P_SIGMA, W, true);
        out(j, NFL_GRD_HEADS + 0, NFL_SEG_NAT, 0, 1);
        in(j, nfl_act_h(nkp, 8), NFL_SEG_ACT, 0, W);
        push(j);
    }
    {   // G | Gt = (delta_dirh | delta_g1) (x) h8 into the scratch: everything that touches `feat` (xyz_encoding_final
        // itself and the first 256 input columns of dir_encoding / transient_encoding.0) is composed from it.
        // Without the transient head there is room for a fifth out tile: the sigma head reads the same h8 (ld 256 too)
        WgJob j = make_job(WG_SCRATCH, W, !ut);
        out(j, NFL_GRD_DIRH, NFL_SEG_ACT, 0, H);
        if (ut) {
            out(j, NFL_GRD_G(1), NFL_SEG_ACT, H, H);
        } else {
            j.bias_layer_of_ot[j.n_ot] = NFL_P_SIGMA;
            out(j, NFL_GRD_HEADS + 0, NFL_SEG_NAT, 0, 1);
        }
        in(j, nfl_act_h(nkp, 8), NFL_SEG_ACT, 0, W);
        push(j);
    }
    {   // dir_encoding: the side inputs [dir PE | appearance] (columns 256..) and the bias
        WgJob j = make_job(NFL_P_DIR, p.ld[NFL_P_DIR], true);
        out(j, NFL_GRD_DIRH, NFL_SEG_ACT, 0, H);
        in(j, nfl_act_d(nkp), NFL_SEG_NAT, W, cd);
        if (p.has_a) in(j, nfl_act_d(nkp) + 2, NFL_SEG_NAT, W + cd, p.n_a);
        push(j);
    }
    {   // rgb head
        WgJob j = make_job(NFL_P_RGB, H, true);
        out(j, NFL_GRD_HEADS + 1, NFL_SEG_NAT, 0, 3);
        in(j, nfl_act_dirh(nkp), NFL_SEG_ACT, 0, H);
        push(j);
    }
    if (ut) {
        {
            WgJob j = make_job(NFL_P_T0, p.ld[NFL_P_T0], true);
            out(j, NFL_GRD_G(1), NFL_SEG_ACT, 0, H);
            in(j, nfl_act_tau(nkp), NFL_SEG_NAT, W, d->n_tau);      // the transient code (columns 256..) and the bias
            push(j);
        }
        for (int m = 2; m <= 4; ++m) {
            WgJob j = make_job(NFL_P_T0 + m - 1, H, true);
            out(j, NFL_GRD_G(m), NFL_SEG_ACT, 0, H);
            in(j, nfl_act_g(nkp, m - 1), NFL_SEG_ACT, 0, H);
            push(j);
        }
        {   // the three transient heads share the g4 stream: one out "tile" each
            WgJob j = make_job(NFL_P_TSIGMA, H, true);
            out(j, NFL_GRD_HEADS + 2, NFL_SEG_NAT, 0, 1);
            out(j, NFL_GRD_HEADS + 3, NFL_SEG_NAT, 0, 3);
            out(j, NFL_GRD_HEADS + 4, NFL_SEG_NAT, 0, 1);
            j.bias_layer_of_ot[0] = NFL_P_TSIGMA;
            j.bias_layer_of_ot[1] = NFL_P_TRGB;
            j.bias_layer_of_ot[2] = NFL_P_TBETA;
            in(j, nfl_act_g(nkp, 4), NFL_SEG_ACT, 0, H);
            push(j);
        }
    }
    if (!ok) return NFL_EINVAL;
    P.n_jobs = nj;
    for (int L = 0; L < NFL_NUM_LAYERS; ++L) {
        const bool tr = L >= NFL_P_T0;
        const int rows = (L <= NFL_P_FINAL) ? W : (L == NFL_P_DIR || (L >= NFL_P_T0 && L < NFL_P_T0 + 4)) ? H
                         : (L == NFL_P_RGB || L == NFL_P_TRGB) ? 3 : 1;
        const bool present = tr ? p.has_t != 0 : true;      // transient layers of the model that this pass does not use get zero gradients
        P.w_numel[L] = present ? rows * p.ld[L] : 0;
        P.b_numel[L] = present ? rows : 0;
    }
    return NFL_OK;
}

// floats of the partial-sum area: WG_MAX_WGS workgroups with the largest accumulator set
static const size_t kPartFloats = (size_t)WG_MAX_WGS * wg_part_len(WG_INST[0][WG_N_INST - 1].nitw);

extern "C" size_t nfl_wgrad_scratch_bytes(void) { return ((size_t)NFL_W * NFL_W + kPartFloats) * sizeof(float); }      // G, then the parts

extern "C" int nfl_wgrad_schedule(const WgPlan* hp, int n_seg, int n_cu, int mult, WgArgs* args, int* n_wg_out, int* n_red_out) {
    if (!hp || hp->magic != WG_PLAN_MAGIC || !args || !n_wg_out || !n_red_out) return NFL_EINVAL;
    const int nj = hp->n_jobs;
    if (nj < 1 || nj > WG_MAX_JOBS || n_seg < 0 || n_cu < 1 || (mult != 1 && mult != 2)) return NFL_EINVAL;
    WgArgs& A = *args;
    A.n_seg = n_seg;
    A.act_rec = hp->act_slots * mult;
    A.grd_rec = hp->grd_slots * mult;
    A.act_lo = mult == 2 ? hp->act_slots * 1024 : 0;
    A.grd_lo = mult == 2 ? hp->grd_slots * 1024 : 0;
    int max_tiles = 1;
    for (int j = 0; j < nj; ++j)
        if (hp->job[j].n_ot + hp->job[j].n_it > max_tiles) max_tiles = hp->job[j].n_ot + hp->job[j].n_it;
    A.slot_bytes = WG_TSTRIDE * max_tiles * mult;
    if (A.slot_bytes > mult * WG_SLOT) return NFL_EINVAL;      // two slots in the dynamic LDS the kernels are given
    // one workgroup per CU, dealt to the jobs in proportion to their streamed bytes
    int total_cost = 0;
    for (int j = 0; j < nj; ++j) total_cost += hp->cost[j];
    if (total_cost < 1) return NFL_EINVAL;
    const int budget = n_cu < WG_MAX_WGS ? n_cu : WG_MAX_WGS;   // one resident workgroup per CU: a second round only repeats the pipeline fill / drain
                                // (measured 1.06 / 1.14 / 1.23 / 1.32 ms for 1 / 2 / 3 / 4 workgroups per CU)
    // proportional shares rounded down, then the workgroups left over go one at a time to the job whose workgroups
    // carry the most bytes each (every CU gets a workgroup and the slowest job sets the kernel's time)
    int n_wg[WG_MAX_JOBS], used = 0;
    for (int j = 0; j < nj; ++j) {
        int n = (int)((long long)budget * hp->cost[j] / total_cost);
        if (n < 1) n = 1;
        if (n > A.n_seg) n = A.n_seg;
        n_wg[j] = n;
        used += n;
    }
    while (used < budget) {
        int best = -1;
        for (int j = 0; j < nj; ++j)
            if (n_wg[j] < A.n_seg && (best < 0 || (long long)hp->cost[j] * n_wg[best] > (long long)hp->cost[best] * n_wg[j])) best = j;
        if (best < 0) break;
        n_wg[best]++;
        used++;
    }
    int acc_wg = 0;
    for (int j = 0; j < nj; ++j) {
        A.wg_start[j] = acc_wg;
        acc_wg += n_wg[j];
    }
    A.wg_start[nj] = acc_wg;
    // partial sums: area of every job's parts, and the reduction's blocks (one per accumulator tile)
    int part_floats = 0, red_blocks = 0;
    for (int j = 0; j < nj; ++j) {
        // the row nfl_wgrad_kernel picks for the job: its NITW is the tile count a part stores
        const int row = wg_inst_row(hp->cost[j], wg_nitw(hp->job[j].n_it, hp->job[j].n_wi));
        if (row < 0) return NFL_EINVAL;
        const int inst = WG_INST[mult - 1][row].nitw;
        A.part_nitw[j] = inst;
        A.part_len[j] = wg_part_len(inst);
        A.part_off[j] = part_floats;
        part_floats += n_wg[j] * A.part_len[j];
        A.red_start[j] = red_blocks;
        red_blocks += 4 * WG_NOT * inst;
    }
    A.red_start[nj] = red_blocks;
    if ((size_t)part_floats > kPartFloats) return NFL_EINVAL;
    *n_wg_out = acc_wg;
    *n_red_out = red_blocks;
    return NFL_OK;
}

int nfl_wgrad_check(const void* h_wplan, const void* d_wplan, const char* d_act_stash, const char* d_grad_stash,
                    const float* d_gmax, int32_t n_rays, int32_t n_samples, int32_t bwd_prec, const nfl_field_params* params,
                    const float* d_scratch, const nfl_field_grads* grads) {
    const WgPlan* hp = static_cast<const WgPlan*>(h_wplan);
    if (!hp || hp->magic != WG_PLAN_MAGIC || !d_wplan || !d_act_stash || !d_grad_stash || !d_gmax || !grads
        || !params || !d_scratch)
        return NFL_EINVAL;
    // the composition reads these master weights; the side-input job of a layer needs its bias gradient as well
    if (!params->weight[NFL_P_FINAL] || !params->bias[NFL_P_FINAL] || !params->weight[NFL_P_DIR]) return NFL_EINVAL;
    const bool ut = wg_plan_transient(hp);
    if (ut && !params->weight[NFL_P_T0]) return NFL_EINVAL;
    if ((grads->weight[NFL_P_DIR] || grads->weight[NFL_P_FINAL]) && !grads->bias[NFL_P_DIR]) return NFL_EINVAL;
    if (ut && (grads->weight[NFL_P_T0] || grads->weight[NFL_P_FINAL]) && !grads->bias[NFL_P_T0]) return NFL_EINVAL;
    if (n_rays < 0 || n_samples < 1) return NFL_EINVAL;
    if (bwd_prec != NFL_PREC_F16 && bwd_prec != NFL_PREC_F16W && bwd_prec != NFL_PREC_F16X3) return NFL_EINVAL;
    if (((uintptr_t)d_scratch | (uintptr_t)params->weight[NFL_P_FINAL]) & 15) return NFL_EINVAL;      // float4 loads along k (G, W_fin rows)
    return NFL_OK;
}

void nfl_wgrad_fill(const WgPlan* hp, const void* d_wplan, const char* d_act_stash, const char* d_grad_stash,
                    const nfl_field_grads* grads, float* d_scratch, WgArgs* args, WgTensors* zero) {
    args->plan = static_cast<const WgPlan*>(d_wplan);
    args->act = d_act_stash;
    args->grd = d_grad_stash;
    args->g = *grads;
    args->scratch = d_scratch;
    args->partial = d_scratch + NFL_W * NFL_W;       // the parts lie behind G
    for (int L = 0; L < NFL_NUM_LAYERS; ++L) {
        zero->ptr[L] = grads->weight[L];
        zero->n[L] = hp->w_numel[L];
        zero->ptr[NFL_NUM_LAYERS + L] = grads->bias[L];
        zero->n[NFL_NUM_LAYERS + L] = hp->b_numel[L];
    }
    zero->ptr[2 * NFL_NUM_LAYERS] = d_scratch;
    zero->n[2 * NFL_NUM_LAYERS] = NFL_W * NFL_W;
}
