// nfl_compose.h -- the composition through xyz_encoding_final as a list of small fp32 products: the task records that
// nfl_wgrad_compose_kernel (nfl_compose.hip) takes by value, and the two builders that fill them (nfl_compose.cpp, plain C++):
// the forward re-pack's fold (nfl_compose_forward) and the gradients nfl_mlp_wgrad composes from G.  g++ builds the pair
// (tests/plan_sweep.cpp runs every task list on host memory under the sanitizers); the .hip units only launch.
#pragma once
#include <stddef.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_wgrad_plan.h"

// Task t computes
//   C[m, n] = sum_k A[m, k] B[k, n] (+ sum_k A2[m, k] B2[k, n]) (+ u[m] v[n]) (+ addm[m]),    m < M, n < N
// over element strides of which one per operand is 1, 32 x 32 output tiles per 256-thread workgroup.
struct WgGemm {
    const float* A; int sam, sak;
    const float* B; int sbk, sbn;
    const float* A2; int sam2, sak2;
    const float* B2; int sbk2, sbn2;
    const float* u; const float* v;       // rank-1 term (NULL: none)
    const float* addm;                    // + addm[m] (NULL: none)
    int avec, bvec;                       // the k-contiguous operand may be fetched with 16-byte loads (rows 16-byte aligned)
    float* Cp; int ldc;
    int M, N, K, K2;                      // K2 = 0: no second product
    int tiles_n, tile0;                   // tiles across N; index of this task's first workgroup
};
#define WG_MAX_GEMM 4
struct WgCompose {
    int n_tasks, n_wg;
    WgGemm t[WG_MAX_GEMM];
};
// passed to the kernel by value: a field that moves changes its scalar loads
static_assert(sizeof(WgCompose) == 552 && offsetof(WgCompose, t) == 8 && offsetof(WgCompose, t[0].tile0) == 136,
              "the compose kernel's kernarg layout");

// Both builders zero *out, fill every field from their inputs and return NFL_OK or NFL_EINVAL; no runtime call.  Before
// NFL_OK they check what the kernel relies on: at most WG_MAX_GEMM tasks, every operand a task reads present, M a multiple
// of 32, K 128 or 256 and K2 0, 128 or 256, ldc >= N, tile0 ascending with n_wg their sum, and for a task with avec / bvec
// set every address the kernel loads as a float4 16-byte aligned (base pointer aligned, row stride a multiple of 4 floats).
//
// The forward fold (nerf_fl_amd.h, nfl_compose_forward): W' = [W[:, :256] W_fin | W[:, 256:]], b' = b + W[:, :256] b_fin for
// dir_encoding.0 and, with has_t, transient_encoding.0: two tasks each.  Refuses a missing pointer and n_side or n_tau < 0.
int nfl_compose_forward_tasks(const nfl_field_params* params, int32_t has_t, int32_t n_side, int32_t n_tau, float* d_wdir_c,
                              float* d_bdir_c, float* d_wt0_c, float* d_bt0_c, WgCompose* out);
// The gradient composition of nfl_mlp_wgrad (nfl_wgrad.hip, file header) from G | Gt in d_scratch: dW_fin, db_fin,
// dW_dir[:, :256] and, when the plan has the transient jobs, dW_t0[:, :256] -- one task per gradient tensor that is given
// (none: n_wg = 0, nothing to launch).  The row strides of W_dir / W_t0 come from the plan's w_numel.
int nfl_compose_backward_tasks(const WgPlan* h_wplan, const nfl_field_params* params, const nfl_field_grads* grads,
                               float* d_scratch, WgCompose* out);
