// nfl_compose.cpp -- the task lists of the composition through xyz_encoding_final (nfl_compose.h).  Plain C++: no runtime
// call here.  The stride tables below are what tests/plan_sweep.cpp evaluates on exactly-sized host blocks.
#include "nfl_compose.h"

#include <string.h>

// appends a task to a composition launch; vec: its k-contiguous operands have 16-byte aligned rows
static void wg_add(WgCompose& Cc, WgGemm g, int vec) {
    g.avec = g.bvec = vec;
    g.tiles_n = (g.N + 31) / 32;
    g.tile0 = Cc.n_wg;
    Cc.n_wg += g.tiles_n * ((g.M + 31) / 32);
    if (Cc.n_tasks < WG_MAX_GEMM) Cc.t[Cc.n_tasks] = g;      // a task too many is counted, not stored: wg_check refuses the list
    ++Cc.n_tasks;
}

static bool wg_rows16(const float* p, int row_stride) { return ((uintptr_t)p & 15) == 0 && row_stride % 4 == 0; }

// what nfl_wgrad_compose_kernel relies on (nfl_compose.h)
static int wg_check(const WgCompose& Cc) {
    if (Cc.n_tasks < 0 || Cc.n_tasks > WG_MAX_GEMM) return NFL_EINVAL;
    int n_wg = 0;
    for (int i = 0; i < Cc.n_tasks; ++i) {
        const WgGemm& g = Cc.t[i];
        if (!g.A || !g.B || !g.Cp || (g.K2 && (!g.A2 || !g.B2)) || (g.u && !g.v)) return NFL_EINVAL;
        if (g.M < 32 || g.M % 32 || g.N < 1 || g.ldc < g.N) return NFL_EINVAL;
        if ((g.K != 128 && g.K != 256) || (g.K2 != 0 && g.K2 != 128 && g.K2 != 256)) return NFL_EINVAL;
        if (g.tiles_n != (g.N + 31) / 32 || g.tile0 != n_wg) return NFL_EINVAL;
        n_wg += g.tiles_n * (g.M / 32);
        // the float4 loads of wg_compose_pass: A along k when sak == 1, B along k when sbk == 1 and sbn != 1
        if (g.avec && g.sak == 1 && !wg_rows16(g.A, g.sam)) return NFL_EINVAL;
        if (g.bvec && g.sbk == 1 && g.sbn != 1 && !wg_rows16(g.B, g.sbn)) return NFL_EINVAL;
        if (g.K2 && g.avec && g.sak2 == 1 && !wg_rows16(g.A2, g.sam2)) return NFL_EINVAL;
        if (g.K2 && g.bvec && g.sbk2 == 1 && g.sbn2 != 1 && !wg_rows16(g.B2, g.sbn2)) return NFL_EINVAL;
    }
    return n_wg == Cc.n_wg ? NFL_OK : NFL_EINVAL;
}

int nfl_compose_forward_tasks(const nfl_field_params* params, int32_t has_t, int32_t n_side, int32_t n_tau, float* d_wdir_c,
                              float* d_bdir_c, float* d_wt0_c, float* d_bt0_c, WgCompose* out) {
    if (!out) return NFL_EINVAL;
    memset(out, 0, sizeof(*out));
    if (!params || !d_wdir_c || !d_bdir_c || (has_t && (!d_wt0_c || !d_bt0_c))) return NFL_EINVAL;
    const float* Wf = params->weight[NFL_P_FINAL];
    const float* bf = params->bias[NFL_P_FINAL];
    if (!Wf || !bf || !params->weight[NFL_P_DIR] || !params->bias[NFL_P_DIR]) return NFL_EINVAL;
    if (has_t && (!params->weight[NFL_P_T0] || !params->bias[NFL_P_T0])) return NFL_EINVAL;
    if (n_side < 0 || n_tau < 0) return NFL_EINVAL;          // they go into a row stride
    const int W = NFL_W, H = NFL_W / 2;
    for (int which = 0; which < (has_t ? 2 : 1); ++which) {
        const int L = which ? NFL_P_T0 : NFL_P_DIR;
        const int ld = W + (which ? n_tau : n_side);
        const float* Ws = params->weight[L];
        WgGemm g;
        memset(&g, 0, sizeof(g));          // W'[r, i] = sum_j W[r, j] W_fin[j, i]   (rows of W are not 16-byte aligned: scalar loads)
        g.A = Ws; g.sam = ld; g.sak = 1; g.B = Wf; g.sbk = W; g.sbn = 1; g.K = W;
        g.Cp = which ? d_wt0_c : d_wdir_c; g.ldc = ld; g.M = H; g.N = W;
        wg_add(*out, g, 0);
        memset(&g, 0, sizeof(g));          // b'[r] = b[r] + sum_j W[r, j] b_fin[j]
        g.A = Ws; g.sam = ld; g.sak = 1; g.B = bf; g.sbk = 1; g.sbn = 1; g.K = W;
        g.addm = params->bias[L];
        g.Cp = which ? d_bt0_c : d_bdir_c; g.ldc = 1; g.M = H; g.N = 1;
        wg_add(*out, g, 0);
    }
    return wg_check(*out);
}

int nfl_compose_backward_tasks(const WgPlan* hp, const nfl_field_params* params, const nfl_field_grads* grads,
                               float* d_scratch, WgCompose* out) {
    if (!out) return NFL_EINVAL;
    memset(out, 0, sizeof(*out));
    if (!hp || hp->magic != WG_PLAN_MAGIC || !params || !grads || !d_scratch) return NFL_EINVAL;
    const bool ut = wg_plan_transient(hp);
    // a rank-1 term or a second product left out for want of its bias gradient would be a wrong gradient, not a refusal
    if ((grads->weight[NFL_P_DIR] || grads->weight[NFL_P_FINAL]) && !grads->bias[NFL_P_DIR]) return NFL_EINVAL;
    if (ut && (grads->weight[NFL_P_T0] || grads->weight[NFL_P_FINAL]) && !grads->bias[NFL_P_T0]) return NFL_EINVAL;
    // G, db_dir, db_t0 are final (unscaled) when the tasks run
    const int W = NFL_W, H = NFL_W / 2;
    const int ld_dir = hp->w_numel[NFL_P_DIR] / H, ld_t0 = ut ? hp->w_numel[NFL_P_T0] / H : 0;
    const float* Wd = params->weight[NFL_P_DIR];
    const float* Wt = ut ? params->weight[NFL_P_T0] : nullptr;
    const float* Wf = params->weight[NFL_P_FINAL];
    const float* G = d_scratch;
    const float* Gt = d_scratch + (size_t)H * W;
    WgGemm g;
    if (grads->weight[NFL_P_FINAL]) {       // dW_fin[i, j] = sum_r Wd[r, i] G[r, j] (+ sum_r Wt[r, i] Gt[r, j])
        memset(&g, 0, sizeof(g));
        g.A = Wd; g.sam = 1; g.sak = ld_dir; g.B = G; g.sbk = W; g.sbn = 1; g.K = H;
        if (ut) { g.A2 = Wt; g.sam2 = 1; g.sak2 = ld_t0; g.B2 = Gt; g.sbk2 = W; g.sbn2 = 1; g.K2 = H; }
        g.Cp = grads->weight[NFL_P_FINAL]; g.ldc = W; g.M = W; g.N = W;
        wg_add(*out, g, 1);      // G and W_fin rows are 1 KiB: float4 loads where k is the contiguous index
    }
    if (grads->bias[NFL_P_FINAL]) {         // db_fin[i] = sum_r Wd[r, i] db_dir[r] (+ sum_r Wt[r, i] db_t0[r]): a 256 x 1 product
        memset(&g, 0, sizeof(g));
        g.A = Wd; g.sam = 1; g.sak = ld_dir; g.B = grads->bias[NFL_P_DIR]; g.sbk = 1; g.sbn = 1; g.K = H;
        if (ut) { g.A2 = Wt; g.sam2 = 1; g.sak2 = ld_t0; g.B2 = grads->bias[NFL_P_T0]; g.sbk2 = 1; g.sbn2 = 1; g.K2 = H; }
        g.Cp = grads->bias[NFL_P_FINAL]; g.ldc = 1; g.M = W; g.N = 1;
        wg_add(*out, g, 1);
    }
    if (grads->weight[NFL_P_DIR]) {         // dW_dir[r, i] = sum_j G[r, j] W_fin[i, j] + db_dir[r] b_fin[i], i < 256
        memset(&g, 0, sizeof(g));
        g.A = G; g.sam = W; g.sak = 1; g.B = Wf; g.sbk = 1; g.sbn = W; g.K = W;
        g.u = grads->bias[NFL_P_DIR]; g.v = params->bias[NFL_P_FINAL];
        g.Cp = grads->weight[NFL_P_DIR]; g.ldc = ld_dir; g.M = H; g.N = W;
        wg_add(*out, g, 1);
    }
    if (ut && grads->weight[NFL_P_T0]) {
        memset(&g, 0, sizeof(g));
        g.A = Gt; g.sam = W; g.sak = 1; g.B = Wf; g.sbk = 1; g.sbn = W; g.K = W;
        g.u = grads->bias[NFL_P_T0]; g.v = params->bias[NFL_P_FINAL];
        g.Cp = grads->weight[NFL_P_T0]; g.ldc = ld_t0; g.M = H; g.N = W;
        wg_add(*out, g, 1);
    }
    return wg_check(*out);
}
