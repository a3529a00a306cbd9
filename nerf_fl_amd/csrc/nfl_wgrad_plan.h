// nfl_wgrad_plan.h -- what the host planner of the weight-gradient pass (nfl_wgrad_plan.cpp, plain C++) and its kernels
// (nfl_wgrad.hip) share: the job list of a field, the launch schedule of a call, the ONE table of the stream kernel's
// instantiations, and the checks and pointer fill of nfl_mlp_wgrad.  Read by g++ and hipcc alike; the kernels read the
// structs and the caller keeps a device copy of the plan.
#pragma once
#include "../../include/nerf_fl_amd.h"
#include "nfl_plan.h"

#define WG_MAX_OT 8      // out tiles (32 features) per job
#define WG_MAX_IT 11     // in tiles per job
#define WG_NOT 2         // out tiles per wave
#define WG_MAX_JOBS 20
#define WG_MAX_WGS 256   // workgroups the partial-sum area is sized for (one per CU)
#define WG_PSTRIDE 1056  // LDS stride of a 1 KiB k-step image: +32 B so the two k-steps of a tile fall on
                         // different banks for the transposed reads (4-way -> 2-way conflicts)
#define WG_TSTRIDE (2 * WG_PSTRIDE)
#define WG_SLOT (WG_TSTRIDE * (WG_MAX_OT + WG_MAX_IT))   // largest LDS slot of a one-product launch; the split kernel's is twice that

struct WgTile {
    int16_t slot;        // first k-step of the tile inside the segment record
    int16_t kind;        // NFL_SEG_ACT / NFL_SEG_NAT
    int16_t idx0;        // row0 / col0 of feature 0 of this tile in the weight
    int16_t nvalid;      // features of this tile that exist (<= 32)
};
#define WG_SCRATCH (-1)   // WgJob::layer of the job that accumulates G | Gt into WgArgs::scratch (256 x 256, ld 256)
struct WgJob {
    int32_t layer;       // NFL_P_* of the weight this job accumulates into, or WG_SCRATCH
    int32_t ld;          // row stride of that weight
    int32_t n_ot, n_it;
    int32_t n_wo, n_wi;  // waves across out tiles / in tiles (n_wo * n_wi == 4)
    int32_t do_bias;
    int32_t bias_layer_of_ot[WG_MAX_OT];   // each out tile may belong to another layer, weight and bias (-1: use `layer`)
    WgTile ot[WG_MAX_OT];
    WgTile it[WG_MAX_IT];
};
struct WgPlan {          // host-built once per (field, transient on/off); the caller keeps a device copy
    uint32_t magic;
    int32_t n_jobs;
    int32_t act_slots, grd_slots;
    int32_t w_numel[NFL_NUM_LAYERS], b_numel[NFL_NUM_LAYERS];   // sizes of the gradient tensors (0: layer absent)
    int32_t cost[WG_MAX_JOBS];     // WgInst::cost of the job's instantiation: 1 KiB pieces per wave per segment, its relative cost
    WgJob job[WG_MAX_JOBS];
};
#define WG_PLAN_MAGIC (NFL_PLAN_MAGIC ^ 0x57u)
struct WgArgs {
    const WgPlan* plan;  // device
    const char* act;     // activation stash
    const char* grd;     // gradient stash
    int n_seg;
    int act_rec, grd_rec;            // slots per segment record of the two stashes (twice the plan's with split stashes)
    int act_lo, grd_lo;              // split stashes: byte offset of the residual record behind the hi record (0: none)
    int slot_bytes;                  // bytes of one LDS slot of this launch (all hi (+ lo) pieces of the largest job)
    int wg_start[WG_MAX_JOBS + 1];   // workgroups [wg_start[j], wg_start[j+1]) work on job j
    nfl_field_grads g;
    float* scratch;      // (256, 256): rows 0..127 G (delta_dirh (x) h8), rows 128..255 Gt (delta_g1 (x) h8)
    // partial sums: workgroup `part` of job j stores its accumulators at partial + part_off[j] + part * part_len[j] (floats), as
    // [(wave * WG_NOT + a) * part_nitw[j] + b][r / 4][lane][r % 4] followed by the bias sums [(wave * WG_NOT + a)][lane]; nfl_wgrad_reduce_kernel
    // adds the parts up in a fixed order, divides by the loss scale and writes the gradient tensors
    float* partial;
    int part_off[WG_MAX_JOBS], part_len[WG_MAX_JOBS], part_nitw[WG_MAX_JOBS];
    int red_start[WG_MAX_JOBS + 1];  // reduction blocks [red_start[j], red_start[j+1]) belong to job j: one per (wave, a, b)
};
// floats of one workgroup's part with `nitw` in tiles per wave: 4 waves x WG_NOT x nitw accumulator tiles, then the bias sums
NFL_HD_EARLY int wg_part_len(int nitw) { return 4 * WG_NOT * nitw * 1024 + 4 * WG_NOT * 64; }

// ---- the instantiations of the stream kernel (wg_body_rs<PW, NITW, D, SPLIT>) and the rule that picks one ----
// A wave of a job loads every fourth 1 KiB piece of a segment (PW of them: 2 per tile, 4 waves) and accumulates WG_NOT x NITW
// tiles; D is the number of segments it keeps in flight, i.e. what the register file holds beside the accumulators.
// The split kernel (NFL_PREC_F16X3) moves the residual pieces too: twice the pieces per segment, fewer segments in flight.
// Its 5-piece class runs with 12 pieces per wave: 10 would do, but that instantiation gave wrong sums on the GPU (not
// understood); 12 is what every gradient fixture verifies.
#ifndef WG_D4            // segments in flight per wave of the one-product kernel, by row class (`make variant` overrides them)
#define WG_D4 8
#define WG_D5 8
#define WG_D6 7
#define WG_D8A 6
#define WG_D8B 5
#endif
// cost: pieces per wave per segment of the one-product kernel, the class of the row and the job's relative cost; then PW, NITW, D
struct WgInst { int cost, pw, nitw, d; };
#define WG_N_INST 7
constexpr WgInst WG_INST[2][WG_N_INST] = {
    {{4, 4, 1, WG_D4}, {4, 4, 2, WG_D4}, {5, 5, 2, WG_D5}, {6, 6, 4, WG_D6}, {8, 8, 5, WG_D8A}, {8, 8, 6, WG_D8A}, {8, 8, 8, WG_D8B}},
    {{4, 8, 1, 4}, {4, 8, 2, 4}, {5, 12, 2, 3}, {6, 12, 4, 3}, {8, 16, 5, 2}, {8, 16, 6, 2}, {8, 16, 8, 2}},      // SPLIT
};
// Row of a job with `pw` hi pieces per wave and `nitw` in tiles per wave: the first one that holds both; -1: none does.
// The planner calls it with the job's piece count and records the row's class in WgPlan::cost; the launch schedule and the
// kernels' dispatcher look the row up again from that class.
constexpr int wg_inst_row(int pw, int nitw) {
    for (int i = 0; i < WG_N_INST; ++i)
        if (pw <= WG_INST[0][i].cost && nitw <= WG_INST[0][i].nitw) return i;
    return -1;
}
NFL_HD_EARLY int wg_nitw(int n_it, int n_wi) { return (n_it + n_wi - 1) / n_wi; }       // in tiles per wave of a job

// The launch schedule of one call: every WgArgs field that is not a pointer, and the grids of the stream and the reduction.
//   n_seg  32-sample segments of the call;  n_cu  compute units of the device;  mult  2 with split (hi + lo) stashes, else 1
// NFL_EINVAL: a plan that nfl_wgrad_plan_build did not make, or one whose parts / LDS slots exceed what the library sizes.
extern "C" int nfl_wgrad_schedule(const WgPlan* h_plan, int n_seg, int n_cu, int mult, WgArgs* args, int* n_wg, int* n_red);

// What nfl_wgrad_zero_kernel clears before the stream (the reduction stores only the elements a job owns).
#define WG_NTENS (2 * NFL_NUM_LAYERS + 1)     // weights, biases, the composition scratch
struct WgTensors {
    float* ptr[WG_NTENS];
    int n[WG_NTENS];
};
// the plan has the transient jobs (its last job is then the transient heads'): the composition takes W_t0 and Gt in
inline bool wg_plan_transient(const WgPlan* hp) {
    return hp->n_jobs > 0 && hp->n_jobs <= WG_MAX_JOBS && hp->job[hp->n_jobs - 1].layer == NFL_P_TSIGMA;
}
// Every refusal of nfl_mlp_wgrad (its arguments; NFL_OK or NFL_EINVAL), the last one the 16-byte alignment of d_scratch and
// params->weight[NFL_P_FINAL] that the composition's float4 loads need.  No runtime call: the entry point makes it first.
int nfl_wgrad_check(const void* h_wplan, const void* d_wplan, const char* d_act_stash, const char* d_grad_stash,
                    const float* d_gmax, int32_t n_rays, int32_t n_samples, int32_t bwd_prec, const nfl_field_params* params,
                    const float* d_scratch, const nfl_field_grads* grads);
// The pointer fields of *args (nfl_wgrad_schedule fills the others) and the zero list of a checked call.
void nfl_wgrad_fill(const WgPlan* h_plan, const void* d_wplan, const char* d_act_stash, const char* d_grad_stash,
                    const nfl_field_grads* grads, float* d_scratch, WgArgs* args, WgTensors* zero);
