/*
 * nerf_fl_amd.h -- C ABI of the MI355X-native NeRF-W ray renderer.
 *
 * This is the drop-in boundary for ONE path of nmerty/nerf-fl: everything that
 * happens inside `render_rays` (reference models/rendering.py:49-289) and the
 * field it evaluates (reference models/nerf.py:6-32, 81-212).  The reference
 * has no FFI of its own (it is pure Python); these are the entry points a
 * ctypes stub in the reference's models/rendering.py would bind (see
 * INTEGRATION.md).  Conventions:
 *
 *   - plain pointers and sizes only; no torch / HIP types in the signatures
 *     (`stream` is a hipStream_t passed as void*),
 *   - every pointer named d_* is DEVICE memory owned by the caller,
 *   - nothing here allocates, frees or synchronises; all work is enqueued on
 *     `stream` (graph-capturable),
 *   - every function returns NFL_OK (0) or a negative NFL_E* code;
 *     nfl_strerror() names it.  The Python shim raises RuntimeError on != 0,
 *     which mirrors the reference's "plain Python exception" convention
 *     (SURVEY.md 8b).
 */
#ifndef NERF_FL_AMD_H
#define NERF_FL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFL_ABI_VERSION 10
#define NFL_GMAX_SLOTS 1024

enum {
    NFL_OK = 0,
    NFL_EINVAL = -1,      /* bad argument (null pointer, size, unsupported config) */
    NFL_ELAUNCH = -2,     /* hipLaunchKernel / hipMemcpyAsync failed             */
    NFL_ENODEV = -3,      /* no gfx950 device / kernel image not loadable         */
    NFL_ESMALL = -4       /* caller-provided buffer too small                     */
};

/* Arithmetic used inside the MLP (everything outside the matrix products --
 * positional encoding, activations, compositing, sampling -- is always fp32). */
#define NFL_STATUS_NONFINITE 1   /* a composited per-ray output of a render pass was NaN / inf                        */
#define NFL_STATUS_RANGE 2       /* a weight or an activation exceeded fp16's range (|x| > 65504) inside the fused MLP */

enum {
    NFL_PREC_F16X3 = 0,   /* fp16 MFMA, operands split hi+lo, 3 products: ~2^-21 relative, fp32-class (default) */
    NFL_PREC_F16   = 1,   /* fp16 MFMA, single product: ~2^-11 relative (fast mode)                               */
    NFL_PREC_F16W  = 2    /* BACKWARD only (bwd_prec): as NFL_PREC_F16, but the gradient chain multiplies by hi + lo weight
                             fragments (two products, the weights to fp32 class): no systematic training-curve offset   */
};

/* One field (reference class NeRF, models/nerf.py:80-151).  W=256, D=8,
 * skips=[4] are fixed, as in every configuration the reference ships. */
typedef struct nfl_field_desc {
    int32_t n_emb_xyz;          /* PosEmbedding freqs for xyz: 1..15 (opt.py:25 default 10; test_phototourism.ipynb 15)  */
    int32_t n_emb_dir;          /* PosEmbedding freqs for dir: 1..4 (opt.py:27 default 4)                                */
    int32_t encode_appearance;  /* NeRF-A head: dir layer sees n_a extra inputs (nerf.py:115,134)             */
    int32_t n_a;                /* 1..48 (opt.py --N_a, default 48)                                           */
    int32_t encode_transient;   /* NeRF-U head (nerf.py:141-151)                                              */
    int32_t n_tau;              /* 1..16 (opt.py --N_tau, default 16)                                         */
    float   beta_min;           /* added after compositing (rendering.py:185)                                 */
    int32_t reserved;
} nfl_field_desc;

/* Device pointers to the fp32 parameters of one field, `nn.Linear` layout
 * (weight = (out,in) row-major, bias = (out)); index with NFL_P_*.
 * Names are the reference's state_dict keys. */
enum {
    NFL_P_XYZ1 = 0,  /* xyz_encoding_1.0 ... xyz_encoding_8.0 = NFL_P_XYZ1 + i */
    NFL_P_FINAL = 8, /* xyz_encoding_final      */
    NFL_P_DIR = 9,   /* dir_encoding.0          */
    NFL_P_SIGMA = 10,/* static_sigma.0          */
    NFL_P_RGB = 11,  /* static_rgb.0            */
    NFL_P_T0 = 12,   /* transient_encoding.0, .2, .4, .6 = NFL_P_T0 + j */
    NFL_P_TSIGMA = 16,
    NFL_P_TRGB = 17,
    NFL_P_TBETA = 18,
    NFL_NUM_LAYERS = 19
};
typedef struct nfl_field_params {
    const float* weight[NFL_NUM_LAYERS];
    const float* bias[NFL_NUM_LAYERS];
} nfl_field_params;

/* ---- plan: static tables describing the packed weight stream ------------ */

/* Bytes of the (host-built, then caller-uploaded) plan for this field. */
size_t nfl_plan_bytes(const nfl_field_desc* desc);
/* Fill `h_plan` (host memory, nfl_plan_bytes) for `prec`.  The caller copies it
 * verbatim to device memory and passes that pointer as d_plan below. */
int nfl_plan_build(const nfl_field_desc* desc, int prec, void* h_plan, size_t bytes);
/* Bytes of the packed weight stream (fp16 MFMA fragments + fp32 bias table). */
size_t nfl_packed_bytes(const nfl_field_desc* desc, int prec);
/* Number of fp32 parameters of the field (sum of numel), for gradient arenas. */
size_t nfl_param_count(const nfl_field_desc* desc);

/* Re-pack the current fp32 parameters into MFMA fragment order (run after every
 * optimizer step; ~2.4 MB read, <=4.8 MB written). h_plan is the same table in
 * HOST memory (used only to size the launch).  d_status (device int32, may be NULL): NFL_STATUS_RANGE is OR-ed in
 * when a weight does not fit fp16's range. */
int nfl_pack_field(const void* h_plan, const void* d_plan, const nfl_field_params* params,
                   void* d_packed, size_t packed_bytes, int32_t* d_status, void* stream);
/* xyz_encoding_final is linear and feeds dir_encoding.0 / transient_encoding.0 only, so the packed streams carry no tiles
 * for it: it is folded into the first 256 input columns of those two layers,
 *   W' = [W[:, :256] W_fin | W[:, 256:]],   b' = b + W[:, :256] b_fin.
 * n_side = side-input columns of dir_encoding.0 = (6 n_emb_dir + 3) + n_a (0 without the appearance input).
 * d_wdir_c (128, 256 + n_side) and d_wt0_c (128, 256 + n_tau; with has_t) must hold COPIES of dir_encoding.0.weight /
 * transient_encoding.0.weight on entry (their side columns are kept); d_bdir_c / d_bt0_c (128) are written.  Pack with a
 * nfl_field_params whose weight / bias entries NFL_P_DIR (and NFL_P_T0) point at these folded tensors; every other
 * entry point (nfl_mlp_wgrad's `params`) takes the ORIGINAL parameters.  One launch, fp32 (v_mfma_f32_32x32x2_f32).
 * NFL_EINVAL, before anything is launched: a pointer that is needed and missing, n_side < 0 or n_tau < 0. */
int nfl_compose_forward(const nfl_field_params* params, int32_t has_t, int32_t n_side, int32_t n_tau,
                        float* d_wdir_c, float* d_bdir_c, float* d_wt0_c, float* d_bt0_c, void* stream);
/* Several streams in one launch (a training step re-packs the forward and the dgrad stream of both fields after every
 * optimizer update).  Same argument meaning and checks as nfl_pack_field, per job. */
#define NFL_PACK_MAX_JOBS 4
typedef struct nfl_pack_job {
    const void* h_plan;
    const void* d_plan;
    const nfl_field_params* params;
    void* d_packed;
    size_t packed_bytes;
    int32_t* d_status;          /* may be NULL */
} nfl_pack_job;
int nfl_pack_fields(int32_t n_jobs, const nfl_pack_job* jobs, void* stream);

/* ---- one rendering pass (reference: inference(), rendering.py:83-226) --- */

/* A pinhole camera from which a pass can generate its rays in the prologue instead of reading a ray matrix (reference
 * datasets/ray_utils.py:5-55, get_ray_directions + get_rays; same arithmetic as nfl_gen_rays): ray r of the pass is
 * pixel pix0 + r in row-major order of a frame `width` pixels wide; direction [(i - cx) / fx, -(j - cy) / fy, -1] (no
 * half-pixel) rotated by c2w[:, :3] and normalised, origin c2w[:, 3], bounds near / far. */
typedef struct nfl_camera {
    float   c2w[12];            /* 3 x 4 row-major */
    float   fx, fy, cx, cy;
    int32_t width, reserved;
    int64_t pix0;
    float   near, far;
} nfl_camera;

typedef struct nfl_pass_args {
    /* geometry */
    const float* d_rays;        /* (R,8): o(3) d(3) near far   (rendering.py:231-233); may be NULL when h_cam / d_cam is set */
    const nfl_camera* h_cam;    /* HOST pointer or NULL: generate the rays of this pass from the camera (copied at launch;
                                   inference only: not with d_act_stash)                                             */
    const float* d_view_dir;    /* (R,3) or NULL -> use rays_d (rendering.py:236-238)  */
    int32_t n_rays;             /* R                                                     */
    int32_t n_samples;          /* samples per ray in THIS pass: N_samples (coarse) or N_samples+N_importance (fine) */
    /* depths: either given (fine pass: sorted output of nfl_sample_pdf) ...      */
    const float* d_z;           /* (R,n_samples) or NULL                                 */
    /* ... or generated in-kernel (coarse pass, rendering.py:243-259)              */
    const float* d_lin;         /* (n_samples) = linspace(0,1,n_samples); required when d_z == NULL */
    const float* d_perturb_rand;/* (R,n_samples) U[0,1) or NULL when perturb == 0         */
    float   perturb;
    int32_t use_disp;
    float*  d_z_out;            /* (R,n_samples) or NULL: the depths actually used       */
    /* density noise (rendering.py:151-152; ignored when the transient head is on) */
    const float* d_noise;       /* (R,n_samples) N(0,1) or NULL                          */
    float   noise_std;
    /* latent codes, already looked up per ray (rendering.py:276-286)              */
    const float* d_a_emb;       /* (R,n_a)  or NULL                                      */
    const float* d_t_emb;       /* (R,n_tau) or NULL -> transient head off for this pass */
    /* mode */
    int32_t sigma_only;         /* coarse pass at test_time (rendering.py:103-111,169)   */
    int32_t white_back;
    int32_t test_extras;        /* test_time on a transient pass: rgb/depth_fine_{static,transient} */
    int32_t stash_split;        /* with d_act_stash: 1 = write split (hi + lo) activation records for a backward in
                                   NFL_PREC_F16X3 (size the stash with nfl_act_stash_bytes(..., NFL_PREC_F16X3)); 0 = hi only */
    /* outputs (any may be NULL = not wanted) */
    float* d_weights;           /* (R,n_samples)                                         */
    float* d_opacity;           /* (R)                                                   */
    float* d_rgb;               /* (R,3)  rgb_coarse / rgb_fine                          */
    float* d_depth;             /* (R)                                                   */
    float* d_transient_sigmas;  /* (R,n_samples)                                         */
    float* d_beta;              /* (R)                                                   */
    float* d_rgb_static;        /* (R,3)  _rgb_fine_static                               */
    float* d_rgb_transient;     /* (R,3)  _rgb_fine_transient                            */
    float* d_rgb_static_only;   /* (R,3)  rgb_fine_static   (test_extras)                */
    float* d_depth_static_only; /* (R)    depth_fine_static                              */
    float* d_rgb_transient_only;/* (R,3)  rgb_fine_transient                             */
    float* d_depth_transient_only;/* (R)  depth_fine_transient                           */
    float* d_field_raw;         /* (R*n_samples,9) per-sample field outputs [rgb,sigma,rgb_t,sigma_t,beta] or NULL;
                                   required (with d_act_stash) when a backward will follow                      */
    char*  d_act_stash;         /* nfl_act_stash_bytes(): fp16 layer inputs of every sample in MFMA fragment order, then
                                   the relu-mask words; consumed by nfl_mlp_dgrad / nfl_mlp_wgrad; NULL for inference */
    /* BARF coarse-to-fine encoding (reference BarfPosEmbedding, nerf.py:35-77): per-frequency weights,
       computed by the caller exactly as barf_weight(freq, epoch) does; NULL = plain PosEmbedding     */
    const float* d_pe_w_xyz;    /* (n_emb_xyz) or NULL                                                   */
    const float* d_pe_w_dir;    /* (n_emb_dir) or NULL                                                   */
    /* NerfWLoss fused into the per-ray epilogue of a TRAINING pass (reference losses.py:35-50): with
       d_loss_target set, every completed ray adds its share of the loss terms to d_losses[4] = {c_l, f_l, b_l, s_l}
       (float atomics, one flush per workgroup; the caller zeroes the array once per step) -- loss_slot 0: this is the
       coarse pass (c_l); 1: the fine pass (f_l, and with the transient head b_l and s_l) -- and writes the backward
       seeds d loss / d rgb (and d loss / d beta) of the ray, which nfl_composite_backward takes as g_rgb / g_beta.
       The caller then needs none of the per-sample outputs (weights, transient_sigmas) for the loss. */
    const float* d_loss_target; /* (R,3) target colours, or NULL = no fused loss                                   */
    float*  d_losses;           /* (4)                                                                              */
    float*  d_seed_rgb;         /* out (R,3)                                                                        */
    float*  d_seed_beta;        /* out (R); fine pass with the transient head only                                  */
    float   loss_coef, lambda_u;/* losses.py:36: coef = 1, lambda_u = 0.01                                          */
    int32_t loss_slot, reserved2;
    /* optional status word (device, int32, never cleared by the library): NFL_STATUS_* bits are OR-ed in.  The MLP
       multiplies fp16 operands: an activation or a weight beyond fp16's range (|x| > 65504), which the fp32 reference
       would carry, cannot be represented here (hi = inf, lo = -inf; the matrix cores then produce NaNs that the next
       relu turns into zeros, so the outputs may even look plausible) -- the ABI's range limit.  The
       kernels track the largest fp16 operand they form and report NFL_STATUS_RANGE; this word is how a caller learns
       of it without scanning anything. */
    int32_t* d_status;
    /* used by nfl_field_forward only (leave NULL / 0 otherwise) */
    const float* d_embedded;
    int32_t n_points, embedded_stride;
    /* the camera in DEVICE memory (same struct as h_cam; takes precedence over it): the launch then carries only the
       pointer, so a pass captured in a HIP graph renders whatever camera the buffer holds at replay time (h_cam is copied
       into the launch's arguments and would be frozen by the capture).  Must not change while the pass runs. */
    const nfl_camera* d_cam;
} nfl_pass_args;

/* Evaluate the field on every sample of every ray and alpha-composite on the
 * fly (one fused kernel; per-sample activations never reach HBM). */
int nfl_render_pass(const void* h_plan, const void* d_plan, const void* d_packed,
                    const nfl_pass_args* args, void* stream);

/* ---- the field alone (reference NeRF.forward, models/nerf.py:153-212) ---------
 * d_x (n_points, row_stride) fp32 = [encoded xyz | encoded dir (+ appearance) | tau], exactly the
 * matrix the reference module takes; d_out (n_points, 9) = [rgb(3), sigma, rgb_t(3), sigma_t, beta]
 * (columns the mode does not compute are written as 0).  Same fused MFMA kernel as the
 * renderer, with the encoding/compositing stages compiled out. */
int nfl_field_forward(const void* h_plan, const void* d_plan, const void* d_packed,
                      const float* d_x, int32_t n_points, int32_t row_stride,
                      int32_t sigma_only, int32_t output_transient, float* d_out, void* stream);
/* reference PosEmbedding / BarfPosEmbedding.forward (models/nerf.py:19-32, 61-77): d_x (n,3) ->
 * d_out (n, 6*n_freqs+3); d_w (n_freqs) BARF weights or NULL */
int nfl_posenc(const float* d_x, int32_t n, int32_t n_freqs, const float* d_w, float* d_out, void* stream);
/* reference datasets/ray_utils.py:5-55 (get_ray_directions + get_rays) for `count` pixels of a frame of width `width`,
 * starting at row-major pixel index `start`: camera direction [(i-cx)/fx, -(j-cy)/fy, -1] (no half-pixel), rotated by
 * c2w[:, :3] and normalised; origin c2w[:, 3].  h_c2w: 12 floats, 3x4 row-major, on the HOST.  d_rays (count, 8) =
 * [origin, direction, near, far], the matrix nfl_render_pass takes. */
int nfl_gen_rays(const float* h_c2w, float fx, float fy, float cx, float cy, int32_t width, int64_t start,
                 int32_t count, float near, float far, float* d_rays, void* stream);

/* ---- backward (training) ---------------------------------------------------
 * The reference gets its gradients from autograd replaying ~100 ATen kernels per
 * point chunk over saved (chunk,256) activations.  Here:
 *   forward (d_act_stash, d_field_raw set)  ->  nfl_composite_backward  ->  nfl_mlp_dgrad
 *   ->  nfl_mlp_wgrad.  All gradients are returned in fp32.  The MLP part of the backward is
 *   mixed precision: fp16 MFMA with fp32 accumulation on activations stashed in fp16 and on
 *   gradients multiplied by a per-pass power-of-two LOSS SCALE, chosen on the device from
 *   max|head gradient| (d_gmax, written by nfl_composite_backward) so that fp16's range is
 *   used whatever the loss magnitude; the scale is divided out before anything is returned.
 *
 *   bwd_prec selects the arithmetic of that MLP part (profiles/r03_psnr_backward_attribution.txt):
 *     NFL_PREC_F16   (default) one fp16 product everywhere: gradients within a few 1e-3 of fp32 autograd per step, fastest;
 *                    the fp16-rounded transposed weights of the chain leave a small systematic offset in long training
 *                    curves (-0.4 .. -1 % of the late training loss on the NeRF-W parity scene; validation PSNR unaffected);
 *     NFL_PREC_F16W  the chain delta_{l-1} = W_l^T delta_l reads hi + lo weight fragments (two products): that offset is
 *                    gone (curve within the reference's own run-to-run scatter); stashes and weight gradients as F16;
 *     NFL_PREC_F16X3 the forward's split-operand arithmetic throughout (hi + lo weights, activations and gradients, three
 *                    products, weight gradients from hi + lo records in one pass): fp32-class gradients, the precision class of the
 *                    reference's autograd; the stashes then hold a second, residual record per segment (twice the bytes),
 *                    written by a forward pass with nfl_pass_args::stash_split = 1.
 *   One value must be used for the stash sizes, the forward pass, the dgrad plan / stream and nfl_mlp_wgrad of a step. */
size_t nfl_act_stash_bytes(const nfl_field_desc* desc, int32_t n_rays, int32_t n_samples, int32_t bwd_prec);
size_t nfl_grad_stash_bytes(const nfl_field_desc* desc, int32_t n_rays, int32_t n_samples, int32_t bwd_prec);
/* dgrad plan / packed stream (transposed weights, fp16); same calling pattern as
 * nfl_plan_build / nfl_pack_field (pack with nfl_pack_field using these plans). */
/* rays_grad != 0: the stream also carries the tiles needed for the gradient w.r.t. the rays
 * (learnable poses, reference models/poses.py + train.py:86-98). */
int    nfl_bwd_plan_build(const nfl_field_desc* desc, int32_t rays_grad, int32_t bwd_prec, void* h_plan, size_t bytes);
size_t nfl_bwd_packed_bytes(const nfl_field_desc* desc, int32_t rays_grad, int32_t bwd_prec);

typedef struct nfl_compbwd_args {
    const float* d_field_raw;       /* (R*N,9) from the forward pass                       */
    const float* d_z;               /* (R,N) depths the forward pass used                  */
    const float* d_noise;           /* (R,N) or NULL, as given to the forward pass         */
    float   noise_std;
    int32_t n_rays, n_samples;
    int32_t use_transient;          /* the forward pass evaluated the transient head       */
    int32_t white_back;
    int32_t reserved;
    /* gradients of the pass outputs; NULL = zero */
    const float* g_weights;         /* (R,N)  */
    const float* g_opacity;         /* (R)    */
    const float* g_rgb;             /* (R,3)  rgb_coarse / rgb_fine                        */
    const float* g_depth;           /* (R)    */
    const float* g_transient_sigmas;/* (R,N)  */
    const float* g_beta;            /* (R)    */
    const float* g_rgb_static;      /* (R,3)  _rgb_fine_static                             */
    const float* g_rgb_transient;   /* (R,3)  _rgb_fine_transient                          */
    float g_tsig_const;             /* added to every element of g_transient_sigmas (s_l's constant gradient coef lambda_u / (R N): no (R,N) array needed) */
    int32_t reserved3;
    const float* d_go;              /* device scalar multiplying every gradient above (the upstream gradient of a fused loss) or NULL = 1 */
    float* d_head_grads;            /* out (R*N,9): d/d pre-activation [rgb,sigma,rgb_t,sigma_t,beta] */
    float* d_gmax;                  /* out (NFL_GMAX_SLOTS = 1024 floats): partial maxima of |head gradient| of this pass (zeroed by the call; the consumers take the max) */
} nfl_compbwd_args;
int nfl_composite_backward(const nfl_compbwd_args* args, void* stream);

typedef struct nfl_dgrad_args {
    const float* d_head_grads;      /* (R*N,9) from nfl_composite_backward                 */
    const char*  d_act_stash;       /* from the forward pass                               */
    char*        d_grad_stash;      /* out, nfl_grad_stash_bytes()                         */
    int32_t n_rays, n_samples;
    int32_t use_transient;
    int32_t dir_is_data;            /* with d_g_rays: the forward pass was given a separate d_view_dir, so the direction encoding
                                       does not depend on the rays (rendering.py:236-238): its gradient is left out of d_g_rays */
    float* d_g_a_emb;               /* (R,n_a)  accumulated into (zero it first) or NULL   */
    float* d_g_t_emb;               /* (R,n_tau) accumulated into (zero it first) or NULL  */
    const int64_t* d_latent_row;    /* (R) or NULL.  When set, d_g_a_emb / d_g_t_emb are the gradients of the latent TABLES
                                       (N_vocab, n_a) / (N_vocab, n_tau) and ray r accumulates into row d_latent_row[r] (= ts[r]):
                                       the scatter-add of nn.Embedding's backward (rendering.py:276-286) happens in this kernel  */
    /* gradient w.r.t. the rays (needs a plan built with rays_grad = 1) */
    float* d_g_rays;                /* (R,8) accumulated into: columns 0..2 origin, 3..5 direction; 6,7 untouched; or NULL */
    const float* d_rays;            /* (R,8) as given to the forward pass                  */
    const float* d_z;               /* (R,N) depths the forward pass used                  */
    const float* d_pe_w_xyz;        /* as given to the forward pass (NULL = ones)          */
    const float* d_pe_w_dir;
    const float* d_gmax;            /* (1024) from nfl_composite_backward: fixes the loss scale of this pass */
    uint32_t rounding_seed;         /* NFL_PREC_F16 / NFL_PREC_F16W round their fp16 gradients STOCHASTICALLY (unbiased; see
                                       nfl_mlp_dgrad below).  The draws are a function of (this seed, the work-item, *d_gmax):
                                       the same seed on the same data reproduces them, another seed gives an independent set */
} nfl_dgrad_args;
/* The gradient chain delta_{l-1} = relu'(h_{l-1}) W_l^T delta_l through the field, from the head gradients down to the
 * latent codes (and the rays), every delta_l left in d_grad_stash for nfl_mlp_wgrad.  Arithmetic by the plan's bwd_prec.
 * Rounding (NFL_PREC_F16 / NFL_PREC_F16W): every fp32 -> fp16 conversion of a gradient is STOCHASTIC (v_cvt_sr_f16_f32: up with
 * probability = the discarded fraction), so that its error is zero-mean and independent between samples and averages out of
 * the weight-gradient sums; NFL_PREC_F16's packed transposed weights are rounded the same way by nfl_pack_field (the draw a
 * hash of the weight's bits and position: deterministic, redrawn when the weight changes).  NFL_PREC_F16X3 carries hi + lo
 * parts instead and rounds to nearest.  (The reference differentiates in fp32: train.py:158-174.) */
int nfl_mlp_dgrad(const void* h_bwd_plan, const void* d_bwd_plan, const void* d_bwd_packed,
                  const nfl_dgrad_args* args, void* stream);

/* fp32 gradient tensors in nn.Linear layout, WRITTEN by nfl_mlp_wgrad (it zeroes them, then a reduction
 * launch stores the sums of its workgroups' parts, added in a fixed order and divided by the loss scale:
 * no atomics); entries may be NULL (layer absent / gradient not wanted). */
typedef struct nfl_field_grads {
    float* weight[NFL_NUM_LAYERS];
    float* bias[NFL_NUM_LAYERS];
} nfl_field_grads;
/* wgrad plan: the list of per-layer streaming GEMM jobs (host-built once per field and
 * transient on/off; the caller uploads it verbatim like the other plans). */
size_t nfl_wgrad_plan_bytes(void);
int    nfl_wgrad_plan_build(const nfl_field_desc* desc, int32_t use_transient, void* h_plan, size_t bytes);
/* d_gmax: the same 1024 floats the dgrad of this pass was given (the stashed gradients carry its loss scale).
 * params / d_scratch: xyz_encoding_final is linear, so neither its output nor the gradient w.r.t. its output is ever
 * stashed; the gradients of xyz_encoding_final and of the first 256 input columns of dir_encoding.0 /
 * transient_encoding.0 are composed, in fp32, from G = sum_s delta_dirh (x) h8 (in d_scratch) and the CURRENT fp32 weights of those layers (`params`: the weights the
 * forward pass ran with; weight[NFL_P_FINAL], bias[NFL_P_FINAL], weight[NFL_P_DIR] and, with the transient head,
 * weight[NFL_P_T0] are read).  grads->bias[NFL_P_DIR] (and [NFL_P_T0]) must be given when any composed gradient is.
 * bwd_prec: the value the stashes were sized and written with.  NFL_PREC_F16 / NFL_PREC_F16W: dW = sum_s d_hi (x) h_hi,
 * one streaming pass; NFL_PREC_F16X3: the stashes hold residual records too and every accumulator gets
 * d_hi (x) h_hi + d_lo (x) h_hi + d_hi (x) h_lo in one pass over both (db = sum_s (d_hi + d_lo)).
 * d_scratch (nfl_wgrad_scratch_bytes() = 68 MB, overwritten; reusable by the next call on the same stream) holds G and the
 * PARTIAL SUMS of the streaming kernel's workgroups: every workgroup stores its accumulators there and a reduction launch adds
 * them up in a fixed order, divides by the loss scale and writes the gradient tensors -- the weight and bias gradients are
 * therefore bit-reproducible from run to run (no atomics), and elements no job owns (heads the call leaves out) are zero.
 * The gradient tensors may be views of one caller-owned flat buffer (nerf_fl_amd.parallel.GradArena): they are written in
 * place, so a collective can run on that buffer right after this call.
 * d_scratch and params->weight[NFL_P_FINAL] must be 16-byte aligned (the composition reads rows of G and of W_fin with
 * 16-byte loads).  Every refusal, this one included, is made before anything is launched: a call that returns NFL_EINVAL
 * has left the gradient tensors untouched. */
size_t nfl_wgrad_scratch_bytes(void);
int nfl_mlp_wgrad(const void* h_wplan, const void* d_wplan, const char* d_act_stash, const char* d_grad_stash,
                  const float* d_gmax, int32_t n_rays, int32_t n_samples, int32_t bwd_prec,
                  const nfl_field_params* params, float* d_scratch, const nfl_field_grads* grads, void* stream);

/* ---- optimiser step (reference utils/__init__.py:30-32: torch.optim.Adam(lr, eps=1e-8), no weight decay, no
 * amsgrad) over up to NFL_ADAM_MAX_TENSORS fp32 tensors in one launch.  `step` is the 1-based count of this update
 * (bias corrections 1 - beta^step); a tensor whose grad pointer is NULL is left untouched. */
#define NFL_ADAM_MAX_TENSORS 64
typedef struct nfl_adam_tensors {
    float*       param[NFL_ADAM_MAX_TENSORS];
    const float* grad[NFL_ADAM_MAX_TENSORS];
    float*       exp_avg[NFL_ADAM_MAX_TENSORS];
    float*       exp_avg_sq[NFL_ADAM_MAX_TENSORS];
    int32_t      numel[NFL_ADAM_MAX_TENSORS];
} nfl_adam_tensors;
int nfl_adam_step(const nfl_adam_tensors* tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                  int32_t step, void* stream);
/* The same update with its scalars in DEVICE memory, for launches captured in a HIP graph (a captured launch freezes
 * by-value arguments): d_hyper = float[4] {lr, beta1, beta2, eps}; *d_step = number of updates already applied to
 * these tensors (the kernel uses *d_step + 1).  bump != 0: a second, one-thread launch then increments *d_step; pass 0
 * for all but the last call when more than NFL_ADAM_MAX_TENSORS tensors share one counter. */
int nfl_adam_step_dev(const nfl_adam_tensors* tensors, int32_t n_tensors, const float* d_hyper, int32_t* d_step,
                      int32_t bump, void* stream);

/* ---- the reference's other optimisers (utils/__init__.py:24-42: --optimizer sgd | adam | radam | ranger with
 * --momentum and --weight_decay) over up to NFL_ADAM_MAX_TENSORS fp32 tensors in one launch.  t = the 1-based step,
 * g the gradient, p the parameter; all per-element arithmetic is fp32, every per-launch scalar is computed in fp64
 * from the fp32 hyper-parameters (in the kernel, for both forms: the eager and the captured launch round alike).
 *   NFL_OPT_SGD     torch.optim.SGD(lr, momentum, dampening=0, weight_decay), no nesterov:
 *                     d = g + wd p;  buf = momentum buf + d (buf starts at 0, so buf = d at t = 1);  p -= lr buf.
 *                     Without a momentum buffer (state0 NULL): p -= lr d.
 *   NFL_OPT_ADAM    torch.optim.Adam(lr, betas, eps, weight_decay), no amsgrad: g += wd p (coupled L2), then
 *                     nfl_adam_step's arithmetic in its order (wd = 0: bit-identical to nfl_adam_step).
 *   NFL_OPT_RADAM   torch_optimizer.RAdam (0.3): v = b2 v + (1-b2) g^2;  m = b1 m + (1-b1) g;
 *                     N_max = 2/(1-b2) - 1;  N = N_max - 2t b2^t/(1-b2^t);  p -= (lr wd) p (decoupled, wd != 0);
 *                     N >= threshold: p -= lr r/(1-b1^t) m/(sqrt(v) + eps),
 *                                     r = sqrt((1-b2^t)(N-4)(N-2) N_max / ((N_max-4)(N_max-2) N));
 *                     otherwise:      p -= lr/(1-b1^t) m.
 *   NFL_OPT_RANGER  torch_optimizer.Ranger (0.3) = RAdam with the test N > threshold, then Lookahead: when t % k == 0,
 *                     slow += alpha (p - slow); p = slow.  (The caller initialises slow to p before the first step.)
 * hyper = float[NFL_OPT_HYPER] {lr, beta1 | momentum, beta2, eps, weight_decay, alpha, k, threshold}; a kind ignores
 * what it does not use.  State: state0 = exp_avg | momentum_buffer, state1 = exp_avg_sq, state2 = slow_buffer.
 * A tensor whose grad pointer is NULL is left untouched.  NFL_EINVAL: NULL tensors / hyper, n_tensors outside
 * [0, NFL_ADAM_MAX_TENSORS], an unknown kind, step < 1, a NULL param or a NULL state the kind needs (SGD: state0 when
 * momentum > 0), a negative momentum, Ranger with k < 1.  No memset or memcpy, no atomics: bit-reproducible. */
#define NFL_OPT_SGD 0
#define NFL_OPT_ADAM 1
#define NFL_OPT_RADAM 2
#define NFL_OPT_RANGER 3
#define NFL_OPT_HYPER 8
typedef struct nfl_optim_tensors {
    float*       param[NFL_ADAM_MAX_TENSORS];
    const float* grad[NFL_ADAM_MAX_TENSORS];
    float*       state0[NFL_ADAM_MAX_TENSORS];   /* exp_avg | momentum_buffer */
    float*       state1[NFL_ADAM_MAX_TENSORS];   /* exp_avg_sq (Adam, RAdam, Ranger) */
    float*       state2[NFL_ADAM_MAX_TENSORS];   /* slow_buffer (Ranger) */
    int32_t      numel[NFL_ADAM_MAX_TENSORS];
} nfl_optim_tensors;
int nfl_optim_step(const nfl_optim_tensors* tensors, int32_t n_tensors, int32_t kind, const float* hyper, int32_t step,
                   void* stream);
/* Graph-capturable form, as nfl_adam_step_dev: d_hyper = float[NFL_OPT_HYPER] in device memory, *d_step = updates
 * already applied (the kernel uses *d_step + 1), bump != 0 increments *d_step after the update.  SGD: a NULL state0
 * means no momentum (the device-side momentum is then not read). */
int nfl_optim_step_dev(const nfl_optim_tensors* tensors, int32_t n_tensors, int32_t kind, const float* d_hyper,
                       int32_t* d_step, int32_t bump, void* stream);

/* ---- NerfWLoss (reference losses.py:35-50) on the renderer's outputs, forward and backward in one launch each.
 * Terms (d_losses[4], zeroed by nfl_loss_forward): c_l, f_l, b_l, s_l; f_l uses beta when d_beta != NULL
 * (then d_rgb_fine is required; b_l and, with d_transient_sigmas, s_l are produced too).
 * nfl_loss_backward writes the gradients of sum_k *d_grad_loss[k] * loss_k (a NULL entry counts as 0) w.r.t. rgb_coarse,
 * rgb_fine, beta and transient_sigmas (the last one is the constant coef*lambda_u/(R*N) per element). */
typedef struct nfl_loss_args {
    const float* d_rgb_coarse;        /* (R,3)                                  */
    const float* d_rgb_fine;          /* (R,3) or NULL (coarse-only rendering)  */
    const float* d_beta;              /* (R) or NULL                            */
    const float* d_transient_sigmas;  /* (R,N) or NULL                          */
    const float* d_target;            /* (R,3)                                  */
    int32_t n_rays, n_samples;        /* n_samples: columns of transient_sigmas */
    float   coef, lambda_u;           /* losses.py:36: coef = 1, lambda_u = 0.01 */
    float*  d_losses;                 /* out (4)                                */
    const float* d_grad_loss[4];      /* device scalars: d total / d {c_l, f_l, b_l, s_l}; NULL = 0 */
    float*  d_g_rgb_coarse;           /* out (R,3)                              */
    float*  d_g_rgb_fine;             /* out (R,3)                              */
    float*  d_g_beta;                 /* out (R)                                */
    float*  d_g_transient_sigmas;     /* out (R,N) or NULL                      */
} nfl_loss_args;
int nfl_loss_forward(const nfl_loss_args* args, void* stream);
int nfl_loss_backward(const nfl_loss_args* args, void* stream);

/* ---- learnable camera poses (--refine_pose; reference models/poses.py, utils/lie_group_helper.py:63-84,
 * datasets/ray_utils.py:29-55) --------------------------------------------------------------------------------
 * Per camera c: c2w = make_c2w(r[c], t[c]) @ init_c2w[c] with Exp(r) = I + sin(n)/n K + (1-cos n)/n^2 K^2,
 * n = |r| + 1e-15, K = skew(r).  Per ray i, with c = d_row_of_id[d_ts[i]]:
 *   d_rays[i] = [c2w[:3, 3], normalize(c2w[:3, :3] . d_rays_cam[i, 0:3]), d_rays_cam[i, 3], d_rays_cam[i, 4]].
 * nfl_pose_rays also writes d_rows[i] = c (int32), or -1 for an id outside [0, n_ids) or a row outside [0, n_cams):
 * such a ray is written as NaN and NFL_STATUS_POSE_ID is OR-ed into *d_status (never an out-of-bounds read).
 * nfl_pose_rays_backward reads d_rows (as the forward left it) and d_g_rays (n_rays, 8) and WRITES d_g_r / d_g_t
 * (n_cams, 3; either may be NULL): every camera is written, 0 when no ray of the batch uses it.  No atomics: one
 * wavefront per camera sums its rays in a fixed order, so two calls on the same inputs are bit-identical. */
#define NFL_STATUS_POSE_ID 4     /* an image id (or its pose row) was outside the pose table: the ray came out as NaN */
typedef struct nfl_pose_args {
    const float*   d_r;           /* (n_cams, 3) axis-angle deltas                                   */
    const float*   d_t;           /* (n_cams, 3) translation deltas                                  */
    const float*   d_init_c2w;    /* (n_cams, 4, 4) or NULL (identity)                               */
    const int64_t* d_row_of_id;   /* (n_ids): image id -> pose row                                   */
    const int64_t* d_ts;          /* (n_rays) image ids                                              */
    const float*   d_rays_cam;    /* (n_rays, cam_stride >= 5): camera-frame direction, near, far     */
    int32_t n_cams, n_ids, n_rays, cam_stride;
    float*         d_rays;        /* forward out: (n_rays, 8) o, d, near, far                         */
    int32_t*       d_rows;        /* forward out / backward in: (n_rays) pose row per ray, -1 = bad  */
    const float*   d_g_rays;      /* backward in: (n_rays, 8)                                        */
    float*         d_g_r;         /* backward out: (n_cams, 3) or NULL                               */
    float*         d_g_t;         /* backward out: (n_cams, 3) or NULL                               */
    int32_t*       d_status;      /* optional status word (NFL_STATUS_POSE_ID)                       */
} nfl_pose_args;
int nfl_pose_rays(const nfl_pose_args* args, void* stream);
int nfl_pose_rays_backward(const nfl_pose_args* args, void* stream);

/* ---- NeRF-W appearance codes of unseen images (test-time optimisation; the paper's Phototourism protocol) ----------
 * With the fields frozen and deterministic sampling, the appearance code a_i of image i enters the fine field only
 * through the appearance columns W_a = dir_encoding.0.weight[:, 256 + cd : 256 + cd + n_a] (cd = 6 n_emb_dir + 3):
 *   Z_s   = pre-activation of dir_encoding.0 at sample s with a zero appearance input          (constant: the cache)
 *   u_i   = W_a a_i;   rgb_s = sigmoid(W_rgb relu(Z_s + u_i) + b_rgb);   rgb_r = sum_s w_s rgb_s (+ 1 - opacity_r)
 * nfl_appearance_cache runs one fine render pass (same arguments and outputs as nfl_render_pass; d_a_emb must hold
 * ZEROS, no transient head, three-product plan only) that also writes Z: d_zcache (n_rays, 128, n_pad) fp32, layout
 * [ray][feature][sample], n_pad >= n_samples a multiple of 64; samples n_samples .. n_pad - 1 are not written.  The
 * pass's d_weights (w_s) and d_opacity are the other inputs of the fit. */
int nfl_appearance_cache(const void* h_plan, const void* d_plan, const void* d_packed, const nfl_pass_args* args,
                         float* d_zcache, int32_t n_pad, void* stream);
/* One fit iteration on the MSE  L = sum_r |rgb_r - target_r|^2 / (3 R), in two launches and no atomics
 * (bit-reproducible), no memset or memcpy (graph-capturable):
 *   fit:    one wavefront per work item (a range of rays of ONE image; the caller groups the rays by image and
 *           lists the items): u_i from the current codes, the forward above on the streamed cache, the backward
 *           dL/dpre_s = (W_rgb^T (w_s g_r . rgb_s . (1 - rgb_s))) . [Z_s + u_i > 0], g_r = 2 (rgb_r - target_r) / (3 R),
 *           summed over the item's samples in registers; writes one 128-float gradient partial and one squared-error
 *           partial per item to d_partials, and rgb_r to d_rgb when that is set;
 *   reduce: per image, the partials of its items in order, then W_a^T: WRITES d_grad (every row; an image without
 *           items gets exact zeros) and *d_loss = L.
 * Weights are read in fp32 from the ORIGINAL parameters (not the folded copies).  NFL_EINVAL: a NULL pointer the
 * call needs, n_pad not a multiple of 64 or < n_samples, n_pad > 256, n_a outside 1..128, sizes < 0. */
typedef struct nfl_appfit_args {
    const float*   d_zcache;       /* (n_rays, 128, n_pad) from nfl_appearance_cache, rays grouped by image            */
    const float*   d_weights;      /* (n_rays, n_samples) w_s of the cache pass                                         */
    const float*   d_opacity;      /* (n_rays) of the cache pass; read only with white_back                             */
    const float*   d_target;       /* (n_rays, 3)                                                                       */
    const int32_t* d_items;        /* (n_items, 3): image, first ray, end ray (exclusive)                               */
    const int32_t* d_image_items;  /* (n_images + 1): items of image i are [d_image_items[i], d_image_items[i + 1])      */
    const float*   d_codes;        /* (n_images, n_a)                                                                   */
    const float*   d_w_dir;        /* dir_encoding.0.weight (128, ld_dir)                                               */
    const float*   d_w_rgb;        /* static_rgb.0.weight (3, 128)                                                      */
    const float*   d_b_rgb;        /* static_rgb.0.bias (3)                                                             */
    int32_t n_rays, n_samples, n_pad, n_items;
    int32_t n_images, n_a, ld_dir, col_a;   /* col_a = 256 + cd: first appearance column of dir_encoding.0            */
    int32_t white_back, reserved;
    float*  d_partials;            /* scratch, nfl_appfit_partials_floats(n_items) floats, overwritten                 */
    float*  d_grad;                /* out (n_images, n_a)                                                               */
    float*  d_loss;                /* out (1)                                                                           */
    float*  d_rgb;                 /* out (n_rays, 3) rgb_r under the current codes, or NULL                            */
} nfl_appfit_args;
size_t nfl_appfit_partials_floats(int32_t n_items);
int nfl_appearance_fit(const nfl_appfit_args* args, void* stream);

/* ---- training batches from uint8 images kept on the device (reference datasets/blender.py:73-101,
 * datasets/phototourism.py:150-183: the all_rays / all_rgbs buffers, never materialised) ------------------------------
 * d_pixels holds the images back to back, each row-major H x W x C uint8 with C = 3 or 4 (an RGBA image starts at a
 * 4-byte-aligned byte offset); d_table holds one nfl_image_rec per image, pix0 ascending from 0 and
 * pix0[i + 1] = pix0[i] + width[i] * height[i].  Work item p in [start, start + count) handles flat pixel
 *   q = p                       (key == 0)
 *   q = perm_{key, n_pixels}(p) (key != 0): a keyed bijection of [0, n_pixels) that is computed, not stored -- a balanced
 *       Feistel network (6 rounds) over 2 h bits, h = max(1, ceil(bits(n_pixels - 1) / 2)), walked until the value is
 *       below n_pixels (at most ~4 evaluations on average).  With x = (L << h) | R, round i maps
 *       (L, R) -> (R, L ^ (mix(R * 0x9E3779B1 + k_i) & (2^h - 1))) in uint32 arithmetic,
 *       mix(v) = v ^= v >> 16, v *= 0x85EBCA6B, v ^= v >> 13, v *= 0xC2B2AE35, v ^= v >> 16  (murmur3's finaliser), and
 *       k_i = low 32 bits of splitmix64's i-th output from state `key`
 *       (z = (state += 0x9E3779B97F4A7C15); z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *       z ^ z >> 31).  It depends on (key, n_pixels) only.
 * The image of q is found by a binary search of pix0, (x, y) from the image's width, and row p - start is written:
 *   d_rays  NFL_LAYOUT_WORLD  (count, 8): origin, unit direction, near, far -- the arithmetic (and the device function) of
 *                             nfl_gen_rays, so the row is bit-identical to that call for the same pose and pixel;
 *           NFL_LAYOUT_CAMERA (count, 5): [(x - cx) / fx, -(y - cy) / fy, -1] (not normalised), near, far -- the
 *                             training layout nfl_pose_rays consumes;
 *   d_ts    (count) int64: the image's id;
 *   d_rgb   (count, 3): c / 255.0f by true division (torchvision's ToTensor); for C = 4 then rgb * a + (1 - a) with every
 *           operation rounded on its own (blender.py:89).
 * Any of the three outputs may be NULL and is then skipped.  One launch.  NFL_EINVAL: args, d_pixels or d_table NULL,
 * n_images < 1, n_pixels outside [1, 2^40), start or count < 0, start + count > n_pixels, an unknown layout. */
enum { NFL_LAYOUT_WORLD = 0, NFL_LAYOUT_CAMERA = 1 };
typedef struct nfl_image_rec {
    int64_t pix0;               /* pixels of all earlier images                           */
    int64_t byte0;              /* byte offset of this image in d_pixels                  */
    int32_t width, height, channels, id;
    float   fx, fy, cx, cy, near, far;
    float   c2w[12];            /* 3 x 4 row-major */
} nfl_image_rec;
typedef struct nfl_gather_args {
    const uint8_t*       d_pixels;
    const nfl_image_rec* d_table;     /* (n_images) */
    int32_t  n_images, layout;
    int64_t  n_pixels, start;
    uint64_t key;
    int32_t  count, reserved;
    float*   d_rays;                  /* out (count, 8 | 5) or NULL */
    int64_t* d_ts;                    /* out (count) or NULL        */
    float*   d_rgb;                   /* out (count, 3) or NULL     */
} nfl_gather_args;
int nfl_gather_batch(const nfl_gather_args* args, void* stream);

/* ---- scoring a rendered image where it lies: PSNR, masked PSNR, SSIM (reference metrics.py; eval.py:196-207,
 * train.py:176-210) and the depth image (utils/visualization.py:10-15) ------------------------------------------------
 * nfl_image_metrics scores the region [x0, x1) x [y0, y1) of a width x height prediction d_pred (height * width, 3) fp32,
 * pixel order, against its ground truth, given in exactly one of two forms:
 *   bank form    d_pixels + d_table + image: the uint8 image `image` of an image bank (above), converted to fp32 by the
 *                device function nfl_gather_batch uses (c / 255.0f; RGBA: rgb * a + (1 - a)); its record must hold the
 *                same width and height (checked on the device: a mismatch reads no pixel and yields NaN results);
 *   tensor form  d_target (height * width, 3) fp32 and an optional d_mask (height * width) uint8.
 * Everything is defined on the cropped images, as if both had been sliced to the region (w x h) first.  clip != 0 clamps
 * the prediction to [0, 1] before anything else (NaN stays NaN).  A pixel is `valid` when alpha > 0 (bank form, RGBA),
 * mask != 0 (tensor form with a mask), always otherwise.  Row `slot` of d_results (n_slots, 8) fp64 receives
 *   [0] sse         sum over the 3 h w elements of (pred - truth)^2, differences and squares in fp64
 *   [1] count       3 h w
 *   [2] sse_valid   [3] count_valid      the same over the valid pixels
 *   [4] ssim_sum    sum of the SSIM map
 *   [5] psnr = -10 log10(sse / count)    (+inf for an exact match)
 *   [6] psnr_valid                       (NaN when no pixel is valid)
 *   [7] ssim = ssim_sum / count
 * SSIM map (kornia 0.4.1's ssim with window 3, as metrics.ssim uses it), per channel, all in fp32:
 *   g = exp(-(k - 1)^2 / (2 * 1.5^2)), k = 0..2, normalised to sum 1;  F(x) = correlation with g (outer) g, border by
 *   reflection without repeating the edge (index -1 -> 1, n -> n - 2);
 *   mu1 = F(p), mu2 = F(t), s1 = F(p p) - mu1^2, s2 = F(t t) - mu2^2, s12 = F(p t) - mu1 mu2,
 *   S = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), C1 = 0.01^2, C2 = 0.03^2,
 *   map = 1 - clamp(1 - S, 0, 1).
 * Optional outputs (NULL: skipped): d_pred_u8 (h, w, 3) uint8 = (uint8)(clamp(pred, 0, 1) * 255) (truncation;
 * eval.py:201-203), d_ssim_map (h, w, 3) fp32.
 * Two launches (tiles -> one partial per workgroup in d_scratch; one workgroup adds them in a fixed order), no atomics,
 * no memset or copy: bit-reproducible and capturable in a HIP graph.  d_scratch: at least
 * nfl_image_metrics_scratch_bytes(h, w) bytes, 8-byte aligned, overwritten.
 * NFL_EINVAL (nothing launched): args / d_pred / d_results / d_scratch NULL, both or neither ground-truth forms, a mask
 * without a target, width or height < 1, height * width >= 2^31, a region outside the image or reversed, a non-empty
 * region narrower or shorter than 2 pixels, slot outside [0, n_slots), image outside [0, n_images), scratch_bytes too
 * small.  An empty region (x0 == x1 or y0 == y1) returns NFL_OK without a launch and leaves the slot untouched. */
typedef struct nfl_metrics_args {
    const float*         d_pred;       /* (height * width, 3)                          */
    const uint8_t*       d_pixels;     /* bank form, or NULL                            */
    const nfl_image_rec* d_table;      /* (n_images), bank form, or NULL                */
    int32_t  n_images, image;
    const float*         d_target;     /* (height * width, 3), tensor form, or NULL     */
    const uint8_t*       d_mask;       /* (height * width), tensor form, or NULL        */
    int32_t  width, height;
    int32_t  x0, x1, y0, y1;
    int32_t  clip, slot;
    double*  d_results;                /* (n_slots, 8) */
    int32_t  n_slots, reserved;
    void*    d_scratch;
    size_t   scratch_bytes;
    uint8_t* d_pred_u8;                /* out (h, w, 3) or NULL */
    float*   d_ssim_map;               /* out (h, w, 3) or NULL */
} nfl_metrics_args;
enum { NFL_METRIC_SSE = 0, NFL_METRIC_COUNT, NFL_METRIC_SSE_VALID, NFL_METRIC_COUNT_VALID, NFL_METRIC_SSIM_SUM,
       NFL_METRIC_PSNR, NFL_METRIC_PSNR_VALID, NFL_METRIC_SSIM, NFL_METRIC_COLUMNS };
size_t nfl_image_metrics_scratch_bytes(int32_t h, int32_t w);     /* 0 for h or w < 1 */
int nfl_image_metrics(const nfl_metrics_args* args, void* stream);

/* nfl_depth_image: the region of a width x height depth map d_depth (height * width) fp32 as an image (h, w, 3) uint8:
 * NaN -> 0, mi / ma = minimum / maximum over the region, x = (d - mi) / (ma - mi + 1e-8f) in fp32 by true division,
 * level = (uint8)(255 * x); the output is the level three times (d_lut NULL) or d_lut[level] of a (256, 3) uint8 table.
 * Two launches (partial minima / maxima into d_scratch, then the image), no atomics.  d_scratch: at least
 * nfl_depth_image_scratch_bytes(h, w) bytes, 4-byte aligned.  NFL_EINVAL: args / d_depth / d_image / d_scratch NULL,
 * sizes and region as above (any non-empty region is allowed), scratch_bytes too small.  Empty region: NFL_OK, no launch. */
typedef struct nfl_depth_args {
    const float*   d_depth;            /* (height * width) */
    int32_t  width, height;
    int32_t  x0, x1, y0, y1;
    const uint8_t* d_lut;              /* (256, 3) or NULL */
    uint8_t* d_image;                  /* out (h, w, 3)    */
    void*    d_scratch;
    size_t   scratch_bytes;
} nfl_depth_args;
size_t nfl_depth_image_scratch_bytes(int32_t h, int32_t w);
int nfl_depth_image(const nfl_depth_args* args, void* stream);

/* ---- depth bounds of a sparse point cloud, per image (reference datasets/phototourism.py:122-131: every point into every
 * camera, points behind it dropped, np.percentile of the depths) ---------------------------------------------------------
 * d_xyz (n_points, 3) fp64 world points; d_row (n_images, 4) fp64, the THIRD row of each image's world-to-camera matrix.
 * The depth of point p in image i is ((x r0 + y r1) + z r2) + r3 in fp64, every operation rounded on its own.  With m the
 * number of points of depth > 0 (NaN depths are not counted) and d_(0) <= .. <= d_(m-1) their sorted depths, the quantile
 * q is numpy's default (`linear`) one: v = q (m - 1), k = floor(v), t = v - k, a = d_(k), b = d_(min(k + 1, m - 1)),
 * result = a + (b - a) t for t < 0.5 and b - (b - a)(1 - t) otherwise, all in fp64.  Outputs:
 *   d_bounds (2, n_images) fp64: row 0 the q_lo quantile, row 1 the q_hi quantile;   d_count (n_images) int32: m.
 * An image with m == 0 gets count 0 and NaN twice; m == 1 gets that depth twice.
 * One launch, one workgroup per image: an exact most-significant-digit radix select over the bit pattern of the positive
 * depths (8 passes of 8 bits, histograms in LDS by integer atomics), the depths recomputed from d_xyz in every pass.  No
 * global scratch, no memset, no allocation, no host synchronisation; every output element is written by a plain store.
 * NFL_EINVAL: a NULL pointer, n_images < 1, n_points outside [1, 2^30], a quantile outside [0, 1] (or NaN). */
typedef struct nfl_bounds_args {
    const double* d_xyz;              /* (n_points, 3) */
    const double* d_row;              /* (n_images, 4) */
    int32_t  n_points, n_images;
    double   q_lo, q_hi;
    double*  d_bounds;                /* out (2, n_images) */
    int32_t* d_count;                 /* out (n_images)    */
} nfl_bounds_args;
int nfl_depth_bounds(const nfl_bounds_args* args, void* stream);

/* ---- surface: the iso-surface of a regular lattice as an indexed triangle mesh (marching tetrahedra; the reference has
 * no counterpart: it renders images only) -----------------------------------------------------------------------------------
 * d_lattice (nz, ny, nx) fp32, x fastest; lattice point (x, y, z) lies at lo[k] + index[k] * spacing[k] (k = x, y, z),
 * computed in fp32 with every operation rounded on its own.  A point is INSIDE when value >= iso; NaN is outside, +-inf
 * compare as usual.
 * Split: a corner of a cell is c = dx | dy << 1 | dz << 2; every cell is cut into the six Kuhn tetrahedra (0, a, a | b, 7),
 * (a, b, c) over the permutations of the axis bits (1, 2, 4) in lexicographic order, which all share the body diagonal 0-7.
 * Every tetrahedron edge joins corners lo and hi with lo a subset of hi; it belongs to the lattice point at corner lo and
 * has the type m = hi ^ lo in 1..7 (1, 2, 4: axis edges; 3, 5, 6: face diagonals; 7: body diagonal).  An edge whose ends
 * differ in the inside test carries ONE vertex, shared by all triangles around it (the mesh is welded):
 *   t = (iso - v_a) / (v_b - v_a) clamped by fminf(fmaxf(t, 0), 1) (a NaN becomes 0), a the owner;  p = p_a + t (p_b - p_a);
 *   normal = n / |n| with n = -(g_a + t (g_b - g_a)), |n| = sqrt((n_x n_x + n_y n_y) + n_z n_z), and 0 unless |n| > 0;
 *   g = gradient of the lattice: (v[i+1] - v[i-1]) / (2 s) per axis, (v[i+1] - v[i]) / s and (v[i] - v[i-1]) / s at the border.
 * Triangles wind so that their normal points from inside to outside; degenerate ones (values equal to iso) are kept.
 * Order: vertices by (owner point in lattice order, m), triangles by (cell in lattice order, tetrahedron, place in the
 * case table of csrc/nfl_surface.hip).  No atomics: the output is bit-reproducible.
 *   nfl_surface_bytes(nx, ny, nz)  scratch size: 4 B per point + 16 B per slab of 256 points of an x-row; 0 for sizes
 *                                  the calls below refuse.
 *   nfl_surface_count   two launches: the crossing edges of every point and the triangles of every cell are counted into
 *                       the scratch and prefix-summed there (exclusive, int64, by a scan kernel of the library); the totals
 *                       go to d_totals[0] = V, d_totals[1] = T.  Reads d_lattice .. d_totals.
 *   nfl_surface_emit    one launch: writes d_vertices (V, 3) fp32, d_normals (V, 3) fp32, d_triangles (T, 3) int32 (indices
 *                       into d_vertices).  It needs the scratch nfl_surface_count left for the SAME lattice, sizes and iso,
 *                       and n_vertices / n_triangles = the totals, which the caller has read back to size the outputs
 *                       (the one host synchronisation of an extraction); no element past them is written.
 * No memset, no copy, no allocation.  d_scratch: 8-byte aligned.
 * NFL_EINVAL: args / d_lattice / d_scratch NULL or misaligned, a size below 2, ny or nz above 65535, more than 2^30 points;
 * count: d_totals NULL; emit: n_vertices > INT32_MAX or 3 n_triangles > INT32_MAX (indices are int32), a negative total, an
 * output NULL that its total needs.  NFL_ESMALL: scratch_bytes below nfl_surface_bytes.  Totals of 0: NFL_OK, no launch. */
typedef struct nfl_surface_args {
    const float* d_lattice;           /* (nz, ny, nx) */
    int32_t  nx, ny, nz;
    float    iso;
    float    lo[3];                   /* position of lattice point (0, 0, 0): x, y, z */
    float    spacing[3];              /* x, y, z */
    void*    d_scratch;
    size_t   scratch_bytes;
    int64_t* d_totals;                /* out (2): V, T (count)                  */
    int64_t  n_vertices, n_triangles; /* emit: the totals, read back by the caller */
    float*   d_vertices;              /* out (V, 3) */
    float*   d_normals;               /* out (V, 3) */
    int32_t* d_triangles;             /* out (T, 3) */
} nfl_surface_args;
size_t nfl_surface_bytes(int32_t nx, int32_t ny, int32_t nz);
int nfl_surface_count(const nfl_surface_args* args, void* stream);
int nfl_surface_emit(const nfl_surface_args* args, void* stream);

/* ---- mesh: cleaning an indexed triangle mesh (connected components, a per-component table, compaction; the reference has
 * no counterpart) ------------------------------------------------------------------------------------------------------------
 * A mesh is d_triangles (T, 3) int32 over V vertices.  Definitions:
 *   - two vertices are CONNECTED when some triangle names both; components are the classes of that relation.  Sharing one
 *     vertex is enough to connect two triangles (a bow-tie is one component); a vertex named by no triangle is a component
 *     of its own; repeated indices inside a triangle are allowed;
 *   - the ROOT of a vertex is the smallest vertex index of its component; components are numbered 0 .. C-1 in ascending
 *     order of root;
 *   - a triangle with any index outside [0, V) is IGNORED by every pass: it connects nothing, belongs to no component, is
 *     never kept, never causes an out-of-range access, and nfl_mesh_label counts it;
 *   - V <= INT32_MAX and 3 T <= INT32_MAX; index arithmetic is 64-bit.
 * Atomics are integer compare-and-swap, add, min and max only, whose results do not depend on the order of arrival: every
 * output is bit-reproducible.  No memset, no copy, no allocation: kernels initialise what they accumulate into, and the
 * caller provides the scratch (8-byte aligned; the *_bytes queries return 0 for sizes the calls refuse).  The prefix sums
 * are taken by a scan of the library: tiles of 2048 elements, the tile sums scanned by the same kernel one level up (three
 * levels cover 2^31 elements) and added back, int32 in, int64 out, a fixed order.
 *
 *   nfl_mesh_label   d_component (V) int32 = the dense id of every vertex; d_totals[0] = C, d_totals[1] = the number of
 *                    ignored triangles.  A lock-free union-find (the larger root is pointed at the smaller by an agent-scope
 *                    compare-and-swap; parent[] is read by agent-scope atomic loads while hooks run), a flatten launch, the
 *                    scan of the root flags, a rank launch.  Scratch nfl_mesh_label_bytes(V, T): 16 B per vertex + tile sums.
 *                    V == 0: NFL_OK, nothing launched, nothing written (C is 0 and every triangle is ignored).
 *   nfl_mesh_stats   the table of the C components from d_component (as nfl_mesh_label wrote it; an id outside [0, C) is
 *                    skipped): d_n_vertices (C) int32; d_n_triangles (C) int32, a triangle counting for the component of its
 *                    FIRST index; d_bounds (C, 2, 3) fp32, per axis the min (row 0) and max (row 1) of the component's
 *                    d_positions (V, 3), taken through the order-preserving integer map of fp32 (-0 < +0), non-finite
 *                    coordinates skipped, +inf / -inf where a component has none.  No float sums, so no areas.  Equal ids
 *                    of a wave are combined before one atomic per distinct id.  No scratch: d_bounds holds the integer keys
 *                    until the last launch decodes them in place.  C == 0: NFL_OK, no launch.
 *   nfl_mesh_compact_count / _emit   compaction under d_keep (C) uint8 (non-zero = keep the component).  A vertex is kept
 *                    when its component is; a triangle when it is not ignored and its three vertices are kept.  count writes
 *                    d_totals[0] = V', d_totals[1] = T' (the caller reads them back to size the outputs: the one host
 *                    synchronisation).  emit, with the SAME arguments and scratch plus n_kept_vertices = V',
 *                    n_kept_triangles = T', writes the kept rows of d_vertices, d_normals, d_colors (each (V, 3) fp32; a
 *                    NULL input is skipped) to d_out_* in their original order, and the kept triangles in their original
 *                    order with indices remapped to the kept vertices, and nothing past the totals it is given.
 *                    emit reads neither d_component nor d_keep but refuses what count refuses, those two included.  What
 *                    it reads from the scratch it checks against V, V' and T': with a scratch that is not the one count
 *                    left it skips triangles, and still reads and writes nothing out of range.
 *                    Scratch nfl_mesh_compact_bytes(V, T): a flag (4 B) and an offset (8 B) per vertex and per triangle,
 *                    then one region of tile sums (8 B per 2048 elements and level) sized for the longer of the two
 *                    scans, which run one after the other and share it.
 * NFL_EINVAL: args NULL, a negative size, V > INT32_MAX or 3 T > INT32_MAX, n_components outside [0, V], a NULL pointer the
 * sizes need, a misaligned scratch, d_totals NULL (label, count), kept totals negative or above V / T, an output NULL that
 * an input and its total need (emit).  NFL_ESMALL: scratch_bytes below the query.  Totals of 0: NFL_OK, no launch. */
typedef struct nfl_mesh_label_args {
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    void*    d_scratch;
    size_t   scratch_bytes;
    int32_t* d_component;             /* out (V) */
    int64_t* d_totals;                /* out (2): C, ignored triangles */
} nfl_mesh_label_args;
size_t nfl_mesh_label_bytes(int64_t n_vertices, int64_t n_triangles);
int nfl_mesh_label(const nfl_mesh_label_args* args, void* stream);

typedef struct nfl_mesh_stats_args {
    const int32_t* d_component;       /* (V) */
    const float*   d_positions;       /* (V, 3) */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles, n_components;
    int32_t* d_n_vertices;            /* out (C) */
    int32_t* d_n_triangles;           /* out (C) */
    float*   d_bounds;                /* out (C, 2, 3) */
} nfl_mesh_stats_args;
int nfl_mesh_stats(const nfl_mesh_stats_args* args, void* stream);

typedef struct nfl_mesh_compact_args {
    const int32_t* d_component;       /* (V) */
    const uint8_t* d_keep;            /* (C) */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles, n_components;
    void*    d_scratch;
    size_t   scratch_bytes;
    int64_t* d_totals;                /* out (2): V', T' (count)                 */
    int64_t  n_kept_vertices, n_kept_triangles;   /* emit: the totals, read back by the caller */
    const float* d_vertices;          /* (V, 3) or NULL */
    const float* d_normals;           /* (V, 3) or NULL */
    const float* d_colors;            /* (V, 3) or NULL */
    float*   d_out_vertices;          /* out (V', 3) */
    float*   d_out_normals;           /* out (V', 3) */
    float*   d_out_colors;            /* out (V', 3) */
    int32_t* d_out_triangles;         /* out (T', 3) */
} nfl_mesh_compact_args;
size_t nfl_mesh_compact_bytes(int64_t n_vertices, int64_t n_triangles);
int nfl_mesh_compact_count(const nfl_mesh_compact_args* args, void* stream);
int nfl_mesh_compact_emit(const nfl_mesh_compact_args* args, void* stream);

/* ---- mesh simplification: uniform vertex clustering of an indexed triangle mesh (the reference has no counterpart) ---------
 * Inputs: d_vertices (V, 3) fp32, d_normals (V, 3) fp32, d_colors (V, 3) fp32 or NULL, d_triangles (T, 3) int32; a scalar
 * cell > 0, an origin (3 doubles) and a placement (NFL_SIMPLIFY_MEAN or NFL_SIMPLIFY_QUADRIC).  Definitions:
 *   CLUSTER of a vertex.  Per axis i = floor(((double)p - origin) / cell), in fp64.  A vertex is VALID when its three
 *     coordinates are finite and every i lies in [-2^20, 2^20); other vertices belong to no cluster.  The key of a valid
 *     vertex is (i + 2^20) | (j + 2^20) << 21 | (k + 2^20) << 42: there is no bounding box, the grid is unbounded and
 *     hashed.  The centre of the cell is origin + (i + 0.5) * cell, in fp64.
 *   NEW VERTEX IDS.  Clusters are numbered 0 .. V'-1 in ascending order of the smallest input vertex index they contain
 *     (the rule by which nfl_mesh_label numbers components).  d_cluster (V) int32 maps an input vertex to its new id, -1
 *     for a vertex that is not valid.
 *   TRIANGLES.  An input triangle with an index outside [0, V) is counted (d_totals[2]) and dropped.  A triangle that names
 *     a vertex which is not valid is dropped; so is one of whose three new ids two are equal.  Among the rest, two
 *     triangles are DUPLICATES when their new-id triples are equal up to rotation; the winding is kept, so a reversed
 *     triple is a different triangle.  Of each set of duplicates the lowest input index survives.  Survivors are emitted in
 *     ascending input index with the new ids in the survivor's own corner order; T' is their count.
 *   ATTRIBUTES of a new vertex.  A cluster with exactly one member keeps that member's position, normal and colour bit for
 *     bit.  Otherwise every sum is taken in int64 fixed point, so that the order of summation cannot matter: a member
 *     contributes llrint(x * 2^30) per component, with x = ((double)p - centre) / cell for positions and x = the component
 *     itself for normals and colours (a non-finite normal or colour component contributes 0; finite ones are taken to be
 *     below 2^31 in magnitude).  With n members:
 *       colour     fl32(sum / (n * 2^30));
 *       normal     the three sums as doubles s, fl32(s / |s|) with |s| = sqrt((s_x s_x + s_y s_y) + s_z s_z), zero when |s| = 0;
 *       position, NFL_SIMPLIFY_MEAN      u~ = sum / (n * 2^30), fl32(centre + cell * u~), every operation fp64 and rounded
 *                                        on its own;
 *       position, NFL_SIMPLIFY_QUADRIC   the regularised quadric-error minimum, in the cell's own coordinates.  The
 *         CONTRIBUTING triangles are the input triangles with three indices in range, three valid corners and a finite,
 *         non-zero area a = |c| / 2, c = (p1 - p0) x (p2 - p0) in fp64 from the fp32 positions; n = c / |c|.  For EACH of
 *         its three corners such a triangle adds to that corner's cluster A += w n n^T (6 numbers) and b += w d n, with
 *         w = a / cell^2, d = -n . u0, u0 = (p0 - the centre of that cluster) / cell, p0 the triangle's FIRST corner.
 *         These nine sums are fp64 (atomic adds on doubles: their order is not fixed).  With mu = NFL_SIMPLIFY_LAMBDA *
 *         trace(A), solve (A + mu I) u = mu u~ - b in fp64 and clamp u per axis to [-0.5, 0.5]; u~ takes the place of u
 *         when trace(A) == 0 or when the solve gives a non-finite number.  The position is fl32(centre + cell * u).
 *         The regularisation bounds the condition number of the system by about 1 / NFL_SIMPLIFY_LAMBDA, so the order of
 *         the fp64 sums moves the result by far less than an fp32 ulp; the clamp keeps a new vertex inside its own cell.
 *   A cluster none of whose triangles survive stays as a vertex that no triangle names.
 *   nfl_mesh_simplify_bytes(V, T)   scratch size, carved by the calls themselves: two open-addressed tables (vertex keys:
 *                    the power of two >= 2 V slots of 8 + 4 B; triangles: the power of two >= 2 T slots of 4 + 4 B), per
 *                    vertex a slot, a flag and a rank (4 + 4 + 8 B), per triangle the rotation-canonical new-id triple, a
 *                    slot, a flag and an offset (12 + 4 + 4 + 8 B), the tile sums of the longer scan, and per vertex the
 *                    accumulators of emit (a count, nine int64, nine doubles: 4 + 72 + 72 B).  0 for sizes the calls refuse.
 *   nfl_mesh_simplify_count   writes d_cluster and d_totals = {V', T', out-of-range triangles, vertices that are not valid}.
 *                    The tables are initialised by a kernel (empty marker: a key of all ones, which no vertex has; -1 for a
 *                    triangle slot).  Vertex keys are inserted by linear probing with a 64-bit compare-and-swap; a per-slot
 *                    atomic minimum of the vertex index names the leader of each cluster; the leader flags are scanned (the
 *                    scan of "mesh") and d_cluster[v] = rank of v's leader.  The triangles are mapped and their canonical
 *                    triples written by one launch; the NEXT launch inserts them into the second table, whose slots are
 *                    claimed write-once by a triangle index and compared through the claimant's canonical triple; a
 *                    per-slot atomic minimum of the triangle index names the survivor; the survivor flags are scanned.
 *                    No thread waits for another: every probe sequence ends at the first empty slot, and both tables are
 *                    at most half full.  Integer atomics only: every output is bit-reproducible.
 *   nfl_mesh_simplify_emit    with the SAME arguments, d_cluster and scratch plus n_out_vertices = V', n_out_triangles = T':
 *                    zeroes the accumulators of V' clusters, adds up (int64 atomic adds; for NFL_SIMPLIFY_QUADRIC a pass
 *                    over the triangles with fp64 atomic adds), then the leader of each cluster writes its row of
 *                    d_out_vertices, d_out_normals and (with d_colors) d_out_colors, solving the 3 x 3 system itself; the
 *                    surviving triangles go to d_out_triangles.  Nothing past V' / T' is written, and what is read from
 *                    the scratch and d_cluster is checked against V' and T' first.
 * No memset, no copy, no allocation, no synchronisation.  d_scratch: 8-byte aligned.
 * NFL_EINVAL: args NULL, a negative size, V > INT32_MAX or 3 T > INT32_MAX, cell not finite and positive, an origin that is
 * not finite, an unknown placement, a NULL pointer the sizes need (d_vertices, d_triangles, d_cluster, d_scratch; count:
 * d_totals; emit: d_normals and an output its total needs), a misaligned scratch, totals negative or above V / T (emit).
 * NFL_ESMALL: scratch_bytes below the query.  V == 0: NFL_OK, nothing launched, nothing written. */
#define NFL_SIMPLIFY_LAMBDA 1e-3
#define NFL_SIMPLIFY_MEAN 0
#define NFL_SIMPLIFY_QUADRIC 1
typedef struct nfl_mesh_simplify_args {
    const float* d_vertices;          /* (V, 3) */
    const float* d_normals;           /* (V, 3) */
    const float* d_colors;            /* (V, 3) or NULL */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    double   cell;
    double   origin[3];               /* x, y, z */
    int32_t  placement;               /* NFL_SIMPLIFY_MEAN / NFL_SIMPLIFY_QUADRIC */
    int32_t  reserved;
    void*    d_scratch;
    size_t   scratch_bytes;
    int64_t* d_totals;                /* out (4): V', T', out-of-range triangles, invalid vertices (count) */
    int32_t* d_cluster;               /* out (V): count writes it, emit reads it */
    int64_t  n_out_vertices, n_out_triangles;     /* emit: V' and T', read back by the caller */
    float*   d_out_vertices;          /* out (V', 3) */
    float*   d_out_normals;           /* out (V', 3) */
    float*   d_out_colors;            /* out (V', 3), with d_colors */
    int32_t* d_out_triangles;         /* out (T', 3) */
} nfl_mesh_simplify_args;
size_t nfl_mesh_simplify_bytes(int64_t n_vertices, int64_t n_triangles);
int nfl_mesh_simplify_count(const nfl_mesh_simplify_args* args, void* stream);
int nfl_mesh_simplify_emit(const nfl_mesh_simplify_args* args, void* stream);

/* ---- mesh smoothing: vertex adjacency, Laplacian / Taubin steps and vertex normals from the triangles of an indexed triangle
 * mesh (the reference has no counterpart) -------------------------------------------------------------------------------------
 * Inputs: d_vertices (V, 3) fp32, d_triangles (T, 3) int32; V <= INT32_MAX, 3 T <= INT32_MAX.  Definitions:
 *   IN-RANGE TRIANGLE.  Its three indices lie in [0, V).  Other triangles are counted (d_totals[2]) and take part in nothing.
 *   INCIDENT ENTRIES of a vertex v.  The numbers e = 3 t + c of every in-range triangle t and corner c in {0, 1, 2} with
 *     tri[t][c] == v, in ascending e; a triangle that names v twice is listed twice.  I = the number of all entries
 *     = 3 x the in-range triangles.
 *   CANDIDATES of v (a multiset).  For every incident entry of v the other two indices of that triangle, leaving out any
 *     that equal v.  The NEIGHBOUR ROW of v: the distinct candidates, each once, in ascending index.  N = the total length
 *     of all rows.
 *   BOUNDARY FLAG.  boundary[v] = 1 when some candidate of v has multiplicity exactly 1 (an edge with a single triangle on
 *     it), else 0.  On a closed manifold every multiplicity is 2; an edge shared by three triangles is not a boundary edge;
 *     a vertex that no triangle names has an empty row and boundary = 0.
 *   A SMOOTHING STEP with factor f.  Positions P are fp32; a step is Jacobi: it reads the buffer of the step before only.
 *     FINITE(v): the three coordinates of v are finite.  pinned(v): the byte of d_pinned is non-zero, or fix_boundary is set
 *     and boundary[v] is.  If !FINITE(v) or pinned(v): P'(v) = P(v) bit for bit.  Otherwise s = (0, 0, 0) in fp64, d = 0; for
 *     each w of the row of v in ascending order with FINITE(w): s += (double)P(w) per component (a sequential sum), d += 1.
 *     d == 0: P'(v) = P(v) bit for bit.  Otherwise m = s / (double)d and P'(v) = fl32(p + f * (m - p)), p = (double)P(v): the
 *     subtraction, the product and the sum each rounded in fp64, no contraction, then ONE rounding to fp32.
 *     A call takes a list of factors, one per step: plain Laplacian with n iterations is lambda n times, Taubin with n
 *     iterations is lambda, mu, lambda, mu, ... over 2 n steps.
 *   VERTEX NORMAL from the triangles.  For each incident entry 3 t + c of v in ascending order: p0, p1, p2 = the corners of t
 *     in the triangle's own order, n_t = (p1 - p0) x (p2 - p0) in fp64 from the fp32 positions, each component the difference
 *     of two separately rounded products (the vector of "mesh simplification"; with the winding of "surface" it points from
 *     inside to outside).  An n_t with a non-finite component or with all components zero contributes nothing.
 *     NFL_NORMALS_AREA adds n_t; NFL_NORMALS_UNIFORM adds n_t / |n_t|, |x| = sqrt((x_x x_x + x_y x_y) + x_z x_z).  The sum s
 *     is sequential fp64 in entry order; the result is fl32(s / |s|).  When |s| = 0 or is not finite the result is the row of
 *     d_fallback_normals bit for bit when that pointer is given, zeros otherwise.
 *   nfl_mesh_adjacency_bytes(V, T)   scratch size of count and emit: per vertex two counters, a degree, two int64 offsets
 *                    and a flag (4 + 4 + 4 + 8 + 8 + 1 B), per triangle the incident entries, the neighbour rows and a sorting
 *                    area (12 + 24 + 24 B), and the tile sums of the scan.  0 for sizes the calls refuse.
 *   nfl_mesh_adjacency_count   writes d_totals = {I, N, out-of-range triangles, boundary vertices} and leaves in the scratch
 *                    what emit needs.  The counters are zeroed by a kernel; a thread per triangle checks the range and
 *                    counts its corners (integer atomic adds); the counts are scanned (the scan of "mesh"); the rows are
 *                    filled through per-vertex cursors in the order of arrival and then SORTED, which is what makes every
 *                    output the same from run to run; the candidates of a vertex are sorted, made distinct and counted, and
 *                    the degrees are scanned.  A row of up to NFL_ADJ_SHORT_ROW incident entries is sorted by one thread;
 *                    a longer one by the whole workgroup (a bitonic sort in LDS up to 8192 words, a rank sort through LDS
 *                    tiles beyond), in the same launch.
 *   nfl_mesh_adjacency_emit    with the SAME arguments and scratch plus n_incident = I and n_neighbors = N: writes
 *                    d_tri_offsets (V + 1) int64 and d_incident (I) int32, d_offsets (V + 1) int64 and d_neighbors (N) int32,
 *                    d_boundary (V) uint8.  Nothing past I / N / V is written, and what is read from the scratch is checked
 *                    against the sizes first.
 *   nfl_mesh_smooth_bytes(V)   one (V, 3) fp32 buffer.  0 for sizes the call refuses.
 *   nfl_mesh_smooth  n_steps in [0, NFL_SMOOTH_MAX_STEPS] steps with the factors[] of the host array, read when the call is
 *                    made; a launch per step between d_scratch and d_out_vertices, so that the LAST step writes
 *                    d_out_vertices whatever the parity; n_steps == 0 copies the input by a kernel.  d_vertices is never
 *                    written (d_out_vertices must be another buffer).  d_boundary may be NULL without fix_boundary, d_pinned
 *                    may be NULL.  Everything read from the CSR is bounded: an offset pair that is not
 *                    0 <= a <= b <= n_neighbors gives an empty row, a neighbour outside [0, V) is skipped like a non-finite
 *                    one, so a CSR that is not this mesh's gives wrong positions and never an access out of range.
 *   nfl_mesh_normals the vertex normals above into d_out_normals (V, 3); incident entries outside [0, 3 T), triangles with
 *                    an index outside [0, V) and offset pairs outside [0, n_incident] are skipped in the same way.
 * No memset, no copy, no allocation, no synchronisation; integer atomics only: every output of the four calls is the same
 * from run to run.  d_scratch: 8-byte aligned.
 * NFL_EINVAL: args NULL, a negative size, V > INT32_MAX or 3 T > INT32_MAX, a NULL pointer the sizes need (d_triangles with
 * T > 0; with V > 0 d_scratch, d_totals (count), the five outputs (emit; d_incident and d_neighbors with I, N > 0), d_vertices,
 * d_offsets, d_out_vertices, d_neighbors with N > 0, d_boundary with fix_boundary, factors with n_steps > 0 (smooth),
 * d_vertices, d_tri_offsets, d_out_normals, d_incident with I > 0 (normals)), a misaligned scratch, d_out_vertices ==
 * d_vertices, an unknown weighting, a factor that is not finite, n_steps outside its range, n_incident outside [0, 3 T],
 * n_neighbors outside [0, 2 n_incident] (emit; smooth and normals: a negative total).
 * NFL_ESMALL: scratch_bytes below the query.  V == 0: NFL_OK, nothing launched, nothing written. */
#define NFL_SMOOTH_MAX_STEPS 1024
#define NFL_ADJ_SHORT_ROW 24
#define NFL_NORMALS_AREA 0
#define NFL_NORMALS_UNIFORM 1
typedef struct nfl_mesh_adjacency_args {
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    void*    d_scratch;
    size_t   scratch_bytes;
    int64_t* d_totals;                /* out (4): I, N, out-of-range triangles, boundary vertices (count) */
    int64_t  n_incident, n_neighbors; /* emit: I and N, read back by the caller */
    int64_t* d_tri_offsets;           /* out (V + 1) */
    int32_t* d_incident;              /* out (I) */
    int64_t* d_offsets;               /* out (V + 1) */
    int32_t* d_neighbors;             /* out (N) */
    uint8_t* d_boundary;              /* out (V) */
} nfl_mesh_adjacency_args;
size_t nfl_mesh_adjacency_bytes(int64_t n_vertices, int64_t n_triangles);
int nfl_mesh_adjacency_count(const nfl_mesh_adjacency_args* args, void* stream);
int nfl_mesh_adjacency_emit(const nfl_mesh_adjacency_args* args, void* stream);

typedef struct nfl_mesh_smooth_args {
    const float* d_vertices;          /* (V, 3) */
    const int64_t* d_offsets;         /* (V + 1) */
    const int32_t* d_neighbors;       /* (N) */
    int64_t  n_vertices, n_neighbors;
    const uint8_t* d_boundary;        /* (V) or NULL */
    const uint8_t* d_pinned;          /* (V) or NULL */
    int32_t  fix_boundary;            /* non-zero: boundary vertices stay */
    int32_t  n_steps;
    const double* factors;            /* HOST, n_steps of them */
    void*    d_scratch;
    size_t   scratch_bytes;
    float*   d_out_vertices;          /* out (V, 3) */
} nfl_mesh_smooth_args;
size_t nfl_mesh_smooth_bytes(int64_t n_vertices);
int nfl_mesh_smooth(const nfl_mesh_smooth_args* args, void* stream);

typedef struct nfl_mesh_normals_args {
    const float* d_vertices;          /* (V, 3) */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    const int64_t* d_tri_offsets;     /* (V + 1) */
    const int32_t* d_incident;        /* (I) */
    int64_t  n_incident;
    int32_t  weighting;               /* NFL_NORMALS_AREA / NFL_NORMALS_UNIFORM */
    int32_t  reserved;
    const float* d_fallback_normals;  /* (V, 3) or NULL */
    float*   d_out_normals;           /* out (V, 3) */
} nfl_mesh_normals_args;
int nfl_mesh_normals(const nfl_mesh_normals_args* args, void* stream);

/* ---- occupancy: empty-space skipping at render time (a bit grid from a lattice, rays clipped to it; the reference has no
 * counterpart: it samples all of [near, far] on every ray) -------------------------------------------------------------------
 * The GRID.  A lattice (nz, ny, nx) as in "surface" has cx = nx - 1, cy = ny - 1, cz = nz - 1 cells; cell (i, j, k) spans the
 * lattice points i .. i + 1, j .. j + 1, k .. k + 1, and lattice plane b of axis k lies at fl(lo[k] + fl(b * spacing[k])).
 * A point is INSIDE when value >= threshold (NaN is outside, +-inf compare as usual).  A cell is occupied at dilation 0 when
 * any of its 8 corners is inside, and at dilation d (0 .. 8) when a cell within Chebyshev distance d is occupied at dilation
 * 0; cells outside the grid do not exist.  Storage: one bit per cell, bit i & 31 of the uint32 word
 * (k * cy + j) * wx + (i >> 5), wx = ceil(cx / 32); the bits past cx in the last word of a row are zero.
 *   nfl_occ_bytes(nx, ny, nz)               size of the bit grid: 4 cz cy wx; 0 for sizes the calls below refuse.
 *   nfl_occ_build_bytes(nx, ny, nz, dilate) scratch of the build: two word arrays of one bit per lattice point (rows padded
 *                                           to words, each array to 16 B); 0 for what nfl_occ_build refuses.
 *   nfl_occ_build    four launches: the point flags are balloted into words, then the box-OR over the window
 *                    [i - d, i + d + 1] of points, cut to the lattice (the 8 corners and the dilation in one), is taken
 *                    separably in bit space: along x by shifts with carries from the neighbouring words, along y and z by
 *                    ORing whole words.  No memset, no copy, no allocation, no atomics: the same input gives the same bits.
 *                    NFL_EINVAL (nothing launched): args / d_lattice / d_scratch / d_bits NULL, d_lattice or d_bits not
 *                    4-byte aligned, d_scratch not 8-byte aligned, a size below 2, ny or nz above 65535, more than 2^30
 *                    points, dilate outside 0 .. 8.  NFL_ESMALL: scratch_bytes below nfl_occ_build_bytes.
 *   nfl_occ_clip_rays   one launch, one thread per ray.  d_rays (R, 8) fp32 rows [o, d, near, far], 16-byte aligned; the
 *                    outputs are d_near_far (R, 2) fp32 (8-byte aligned) and d_hit (R) uint8; nothing past R is written.
 *                    Every operation below is fp32 and rounded on its own.  Per ray:
 *                      a NaN among its 8 numbers: a miss.
 *                      slab test against the box lo .. plane c of every axis (c = cx, cy, cz): t0 = near, t1 = far; per axis
 *                        with d != 0: inv = 1 / d, ta = (lo - o) * inv, tb = (plane_c - o) * inv, t0 = fmaxf(t0, fminf(ta,
 *                        tb)), t1 = fminf(t1, fmaxf(ta, tb)); an axis with d == 0 misses unless lo <= o <= plane_c.  The ray
 *                        misses unless t0 < t1.  Space outside the box is empty.
 *                      entry cell: floorf(((o + t0 * d) - lo) / spacing) per axis, clamped to [0, c - 1] by fmaxf / fminf
 *                        before the conversion to an integer.
 *                      walk (Amanatides-Woo): the next plane of an axis is b = cell + (d > 0 ? 1 : 0), its parameter
 *                        ((lo + b * spacing) - o) * inv, recomputed from the integer b at every step (never accumulated),
 *                        +inf where d == 0.  t_out is the smallest of the three, ties to the lowest axis.  An occupied cell
 *                        sets t_first = the parameter it was entered at (t0 for the entry cell, else the t_out of the step
 *                        before) if none was met before, and t_last = fminf(t_out, t1).  The walk ends unless t_out < t1, or
 *                        when the step along that axis leaves the grid: at most cx + cy + cz + 1 cells.
 *                      hit = 1, near' = t_first, far' = t_last when an occupied cell was met and t_last > t_first; otherwise
 *                        hit = 0 and near, far are passed through unchanged.  |d| need not be 1: t is the ray's own depth
 *                        parameter, the one the render kernel samples.
 *                    R == 0: NFL_OK, no launch.  NFL_EINVAL (nothing launched): args NULL, sizes as above, a spacing that is
 *                    not positive and finite, a lo that is not finite, R < 0 or above INT32_MAX, a NULL or misaligned
 *                    pointer. */
typedef struct nfl_occ_build_args {
    const float* d_lattice;           /* (nz, ny, nx) */
    int32_t  nx, ny, nz;
    float    threshold;
    int32_t  dilate;                  /* 0 .. 8 */
    int32_t  reserved;
    void*    d_scratch;
    size_t   scratch_bytes;
    uint32_t* d_bits;                 /* out (cz, cy, wx) */
} nfl_occ_build_args;
size_t nfl_occ_bytes(int32_t nx, int32_t ny, int32_t nz);
size_t nfl_occ_build_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t dilate);
int nfl_occ_build(const nfl_occ_build_args* args, void* stream);

typedef struct nfl_occ_clip_args {
    const float* d_rays;              /* (R, 8) */
    int64_t  n_rays;
    const uint32_t* d_bits;           /* (cz, cy, wx) */
    int32_t  nx, ny, nz;              /* of the LATTICE the grid was built from */
    float    lo[3];                   /* position of lattice point (0, 0, 0): x, y, z */
    float    spacing[3];              /* x, y, z */
    int32_t  reserved;
    float*   d_near_far;              /* out (R, 2) */
    uint8_t* d_hit;                   /* out (R)    */
} nfl_occ_clip_args;
int nfl_occ_clip_rays(const nfl_occ_clip_args* args, void* stream);

/* ---- mesh colour: a depth map of a mesh per camera, and the bank's pixels blended into per-vertex colours (the line of
 * projects this one follows colours an exported mesh the same way: project, test visibility, average) ------------------------
 * Every operation below is fp32 and rounded on its own; dot(a, x) stands for (a0 * x0 + a1 * x1) + a2 * x2 and cross for
 * (a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0).  Divisions and square roots are correctly rounded.
 * The CAMERA is one nfl_image_rec: R[r][c] = c2w[4 r + c], t[r] = c2w[4 r + 3].  A world point p has the camera coordinates
 *   q[c] = dot((R[0][c], R[1][c], R[2][c]), p - t),
 * and pixel (i, j), column i and row j, has the camera-space ray d = ((i - cx) / fx, -(j - cy) / fy, -1): the expressions of
 * nfl_gather_batch's camera layout, pixel centres on the integers.  A run is the images first .. first + count - 1 of a table;
 * pixel (i, j) of image n of the run is word pix0[n] - pix0[first] + j * width + i of the run's depth buffer.
 *
 * nfl_mesh_depth   two launches (fill, raster).  The value of a pixel is the minimum over all triangles its ray hits of the
 *   distance from the camera centre to the hit, +inf when there is none.  With a, b, c the camera coordinates of a triangle's
 *   vertices (Moeller-Trumbore from the origin): tv = -a, e1 = b - a, e2 = c - a, qv = cross(tv, e1), tnum = dot(e2, qv);
 *   per pixel pv = cross(d, e2), det = dot(e1, pv), a miss when det == 0 (or NaN), inv = 1 / det, u = dot(tv, pv) * inv,
 *   v = dot(d, qv) * inv, tau = tnum * inv; a HIT when u >= 0, v >= 0, u + v <= 1 and tau > 0 (two-sided, edges included),
 *   its distance tau * sqrt((dx dx + dy dy) + dz dz).  A triangle with a non-finite camera coordinate, or an index outside
 *   [0, n_vertices) (indices are NOT trusted), hits nothing.  Which pixels a triangle is tried against is the kernel's
 *   business: none when all three vertices have -q.z <= 0; the bounding box of the projections cx + fx * (q.x / s),
 *   cy - fy * (q.y / s), s = -q.z, widened by one pixel each way and cut to the frame, when all three have s > 0 and finite
 *   projections; the whole frame otherwise.  Boxes of more than 64 pixels are walked by a whole wave, in the same launch.
 *   A hit is an atomicMin on the word as uint32 (non-negative floats order as their bits): the result does not depend on the
 *   order.  Only words below n_depth are written; n_depth = the pixels of the run.  V == 0 or T == 0 or count == 0: the fill
 *   alone.  NFL_EINVAL (nothing launched): args / d_table NULL or d_table not 8-byte aligned, n_images < 1, a run outside the
 *   table, a negative size, V > INT32_MAX or 3 T > INT32_MAX, n_depth above 2^38, a NULL or misaligned (4 B) pointer that a
 *   non-zero size needs, more than 2^31 workgroups of 256 (triangle, image) pairs.
 *
 * nfl_mesh_blend   one launch, one thread per vertex, the images of the run in increasing n inside.  For vertex p with normal
 *   nrm, image n contributes when all of these hold:
 *     1  wi = d_image_weights[n] > 0 (NULL: 1 for every image; the array is indexed by the TABLE's n);
 *     2  s = -q.z > 0;
 *     3  u = cx + fx * (q.x / s), v = cy - fy * (q.y / s) with 0 <= u <= width - 1 and 0 <= v <= height - 1 (NaN fails);
 *     4  e = t - p, dist = sqrt(dot(e, e)), cos = dot(nrm, e) / dist > min_cos; a normal of three zeros counts as cos = 1;
 *     5  dist <= depth[floorf(u + 0.5f), floorf(v + 0.5f)] + depth_tol, the depth word of this run's nfl_mesh_depth;
 *     6  with d_center: max_k |c_k - center_k| <= reject.
 *   c is the bilinear sample at (u, v): x = floorf(u), tx = u - x, sx = 1 - tx, likewise y, ty, sy; the neighbours x + 1 and
 *   y + 1 are clamped to the last column and row; c = (c00 * sx + c10 * tx) * sy + (c01 * sx + c11 * tx) * ty with c00 at
 *   (x, y), c10 at (x + 1, y), c01 at (x, y + 1), every pixel converted by the device function of nfl_gather_batch
 *   (c / 255.0f; RGBA: rgb * a + (1 - a)).  The image adds w * c to d_sum[v][0..2], w to d_sum[v][3] and 1 to d_views[v],
 *   w = wi * cos (NFL_BLEND_COS) or wi (NFL_BLEND_UNIFORM).  start != 0 begins the accumulators at zero, start == 0 continues
 *   what the caller's arrays hold, so a bank may be walked in runs; the result does not depend on the split.  No atomics.
 *   NFL_EINVAL (nothing launched): args NULL, V < 0 or above INT32_MAX, d_table / run as above, an unknown weighting,
 *   depth_tol negative or NaN, min_cos NaN (or negative with NFL_BLEND_COS: a weight is never negative), reject negative or NaN
 *   when d_center is given, n_depth as above, and for V > 0 a NULL d_vertices / d_normals / d_sum / d_views (d_pixels, d_depth
 *   when count > 0) or a misaligned pointer (d_sum 16 B, the others 4 B).  V == 0, or count == 0 with start == 0: NFL_OK, no
 *   launch. */
enum { NFL_BLEND_COS = 0, NFL_BLEND_UNIFORM = 1 };
typedef struct nfl_mesh_depth_args {
    const float*   d_vertices;        /* (V, 3) world */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    const nfl_image_rec* d_table;     /* (n_images) */
    int32_t  n_images, first, count, reserved;
    float*   d_depth;                 /* out (n_depth) */
    int64_t  n_depth;                 /* pixels of the run */
} nfl_mesh_depth_args;
int nfl_mesh_depth(const nfl_mesh_depth_args* args, void* stream);

typedef struct nfl_mesh_blend_args {
    const float*   d_vertices;        /* (V, 3) */
    const float*   d_normals;         /* (V, 3) */
    int64_t  n_vertices;
    const uint8_t* d_pixels;
    const nfl_image_rec* d_table;     /* (n_images) */
    int32_t  n_images, first, count, weighting;
    const float*   d_depth;           /* (n_depth): nfl_mesh_depth of the same run */
    int64_t  n_depth;
    const float*   d_image_weights;   /* (n_images) or NULL */
    const float*   d_center;          /* (V, 3) or NULL */
    float    min_cos, depth_tol, reject;
    int32_t  start;                   /* != 0: the accumulators begin at zero */
    float*   d_sum;                   /* in/out (V, 4): sum of w * rgb, sum of w */
    int32_t* d_views;                 /* in/out (V) */
} nfl_mesh_blend_args;
int nfl_mesh_blend(const nfl_mesh_blend_args* args, void* stream);

/* ---- mesh render: a coloured mesh as images -- which triangle wins each pixel, and its vertex attributes interpolated there --
 * Camera, run, pixel ray, dot, cross and the Moeller-Trumbore arithmetic are those of "mesh colour" above, word for word: every
 * operation fp32 and rounded on its own, divisions and square roots correctly rounded.  Pixel (i, j) of image n of the run is
 * word pix0[n] - pix0[first] + j * width + i of the run's buffers.
 *
 * nfl_mesh_visibility   two launches (fill, raster).  The word of a pixel is the minimum, over all triangles tr whose ray test
 *   is a HIT (as defined for nfl_mesh_depth) with a distance d = tau * |ray| below +inf, of
 *     ((uint64_t)bits(d) << 32) | (uint32_t)tr,
 *   and 2^64 - 1 when there is none.  tr is the triangle's index in d_triangles (culled and refused triangles keep their
 *   numbers).  The distance decides; among equal distances the lowest index wins, so the result does not depend on the order
 *   of the hits.  A hit is a 64-bit atomicMin on the word.  Which triangles are tried against which pixels, the 64-pixel
 *   threshold and the whole-wave walk of larger boxes are those of nfl_mesh_depth.  Only words below n_vis are written; n_vis
 *   = the pixels of the run.  V == 0 or T == 0 or count == 0: the fill alone.  NFL_EINVAL (nothing launched): the refusals of
 *   nfl_mesh_depth, with d_vis 8-byte aligned.
 *
 * nfl_mesh_shade   one launch, a thread per word of the run.  The image of a word is found by a binary search of pix0 (as in
 *   nfl_gather_batch), its pixel (i, j) from the image's width.  A word is UNCOVERED when it is 2^64 - 1, when its low half is
 *   not below n_triangles, when that triangle has an index outside [0, n_vertices), when the word lies past the pixels of its
 *   image, count == 0, or when det == 0 (or NaN) for that triangle and pixel (the buffer is the caller's and is not trusted;
 *   no word nfl_mesh_visibility writes is uncovered by the last three).  For a covered word the three vertices are
 *   transformed and u, v and the distance recomputed by the expressions of the raster (the same bits); the hit conditions are
 *   not tested again.  w0 = (1 - u) - v, and an attribute triple A, B, C of the triangle's vertices interpolates to
 *   (w0 * A + u * B) + v * C.  mode:
 *     NFL_SHADE_COLOR    d_attr (V, 3) interpolated; the float result is not clamped.
 *     NFL_SHADE_NORMAL   d_attr holds vertex normals; the interpolated m becomes 0.5f * (m_k / sqrt(dot(m, m))) + 0.5f, and
 *                        0.5 in all three when that length is zero or NaN.
 *     NFL_SHADE_FACING   no attributes: with n = cross(e1, e2) and the pixel's ray d,
 *                        g = |dot(n, d)| / (sqrt(dot(n, n)) * sqrt(dot(d, d))), NaN -> 0, the colour (g, g, g): a headlight.
 *   Outputs, each skipped when NULL: d_rgb (n_vis, 3) fp32; d_rgb_u8 (n_vis, 3) = (uint8_t)(clamp(c, 0, 1) * 255), truncated,
 *   NaN -> 0; d_depth (n_vis) fp32, the distance, bit-equal to nfl_mesh_depth of the same inputs; d_triangle (n_vis) int32.
 *   An uncovered word gets background[3], +inf and -1.  NFL_EINVAL (nothing launched): args / d_table NULL or d_table not
 *   8-byte aligned, n_images < 1, a run outside the table, a negative size, V > INT32_MAX or 3 T > INT32_MAX, an unknown mode,
 *   d_attr NULL in a mode that reads it (and V > 0), n_vis above 2^38, d_vis NULL (n_vis > 0) or not 8-byte aligned, a NULL
 *   d_vertices / d_triangles that a non-zero size needs, another pointer not 4-byte aligned (d_rgb_u8: bytes, any address).
 *   n_vis == 0: NFL_OK, no launch. */
enum { NFL_SHADE_COLOR = 0, NFL_SHADE_NORMAL = 1, NFL_SHADE_FACING = 2 };
typedef struct nfl_mesh_visibility_args {
    const float*   d_vertices;        /* (V, 3) world */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    const nfl_image_rec* d_table;     /* (n_images) */
    int32_t  n_images, first, count, reserved;
    uint64_t* d_vis;                  /* out (n_vis), 8-byte aligned */
    int64_t  n_vis;                   /* pixels of the run */
} nfl_mesh_visibility_args;
int nfl_mesh_visibility(const nfl_mesh_visibility_args* args, void* stream);

typedef struct nfl_mesh_shade_args {
    const float*   d_vertices;        /* (V, 3) world */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    const nfl_image_rec* d_table;     /* (n_images) */
    int32_t  n_images, first, count, mode;
    const uint64_t* d_vis;            /* (n_vis): nfl_mesh_visibility of the same run */
    int64_t  n_vis;
    const float*   d_attr;            /* (V, 3) colours or normals; NULL with NFL_SHADE_FACING */
    float    background[3];
    int32_t  reserved;
    float*   d_rgb;                   /* out (n_vis, 3) or NULL */
    uint8_t* d_rgb_u8;                /* out (n_vis, 3) or NULL */
    float*   d_depth;                 /* out (n_vis) or NULL */
    int32_t* d_triangle;              /* out (n_vis) or NULL */
} nfl_mesh_shade_args;
int nfl_mesh_shade(const nfl_mesh_shade_args* args, void* stream);

/* ---- mesh atlas: a texture for a mesh, baked from the images and sampled by the shading pass ---------------------------------
 * Every operation fp32 and rounded on its own, divisions and square roots correctly rounded, as in "mesh colour" and "mesh
 * render", whose camera, run, visibility words and ray arithmetic are used word for word.
 *
 * THE ATLAS of a mesh of T triangles has one chart per triangle, two triangles to a square cell, all cells the same size; it
 * needs no parameterisation solver.  cell = C texels with 6 <= C <= 1024, L = C - 5; cols >= 1, rows >= 1 and
 * 2 * cols * rows >= T.  It is W = cols * C by H = rows * C texels, row-major, row 0 first, three colours a texel, and
 * W * H <= INT32_MAX.  Texel e is column X = e % W of row Y = e / W; its cell is k = (Y / C) * cols + X / C, its local
 * coordinates i = X % C, j = Y % C; its half is h = 0 when i + j <= C - 1, else 1; its triangle is tr = 2 k + h.
 *   Barycentrics of a texel.  Half 0: u = (float)(i - 1) / (float)L, v = (float)(j - 1) / (float)L.  Half 1 is the cell turned
 *   by 180 degrees: u = (float)((C - 2) - i) / (float)L, v = (float)((C - 2) - j) / (float)L.  w0 = (1 - u) - v, and an
 *   attribute triple A, B, C of the triangle's vertices interpolates to (w0 * A + u * B) + v * C (nfl_mesh_shade's
 *   expression).  Texels outside the triangle (u < 0, v < 0 or u + v > 1) keep these extrapolated barycentrics, NOT clamped:
 *   they are the gutter, and extrapolation is what makes a bilinear lookup reproduce an affine colour up to the hypotenuse.
 *   Surface position.  The point (u, v) of triangle tr has the local coordinates lx = 1 + u * L, ly = 1 + v * L, and in half 1
 *   lx = (float)(C - 1) - lx, ly = (float)(C - 1) - ly.  With u >= 0, v >= 0, u + v <= 1 the bilinear lookup at (lx, ly)
 *   reads with non-zero weight only texels of its own half, all inside the cell.  The corners of the triangle lie ON texels:
 *   (1, 1), (C - 4, 1), (1, C - 4) in half 0; (C - 2, C - 2), (3, C - 2), (C - 2, 3) in half 1.
 *   A texel is OWNERLESS when tr >= T or when its triangle has an index outside [0, n_vertices): indices are not trusted.
 *
 * nfl_atlas_points   one launch, a thread per texel first_texel .. first_texel + n_texels - 1 (a large atlas may be baked in
 *   pieces; the result does not depend on the split).  Row n of the outputs belongs to texel first_texel + n: d_points the
 *   interpolated position, d_normals the interpolated vertex normal m divided by sqrt(dot(m, m)), three zeros when that
 *   length is zero or NaN (nfl_mesh_blend counts a zero normal as cos = 1).  An ownerless texel gets three NaNs and three
 *   zeros: nfl_mesh_blend leaves a NaN point out at its condition 2, so the rows go to it as they are, with no mask.
 *
 * nfl_atlas_resolve   one launch, a thread per texel of the same range, d_sum (n_texels, 4) and d_views (n_texels) being what
 *   nfl_mesh_blend left for nfl_atlas_points' rows.  Ownerless: background[3] (whatever d_views holds).  Seen, d_views > 0:
 *   fminf(fmaxf(sum_k / sum_3, 0), 1), so NaN -> 0.  Unseen with an owner: d_vertex_colors (V, 3) interpolated by the
 *   texel's barycentrics, not clamped, when that pointer is given; fallback[3] otherwise.  Outputs, each skipped when NULL:
 *   d_texture (n_texels, 3) fp32; d_texture_u8 (n_texels, 3) = (uint8_t)(clamp(c, 0, 1) * 255), truncated, NaN -> 0, the rule
 *   of nfl_mesh_shade; d_seen (n_texels) bytes, 1 for a seen texel with an owner, else 0.
 *
 * nfl_mesh_shade_atlas   nfl_mesh_shade in NFL_SHADE_COLOR with the colour taken from the atlas: the uncovered rules, the
 *   recomputation of u, v and the distance, the four outputs and the background are that entry point's.  Exactly one of
 *   d_atlas (fp32 (H, W, 3)) and d_atlas_u8 (bytes, a texel converts by c / 255.0f) is non-NULL.  For a covered word of
 *   triangle tr, lx and ly as above, then clamped into the cell by fminf(fmaxf(., 0), C - 1) (NaN -> 0: a forged word gives
 *   arbitrary barycentrics and still reads inside its cell); x = floorf(lx), tx = lx - x, sx = 1 - tx, likewise y, ty, sy; the
 *   neighbours x + 1 and y + 1 are clamped to C - 1; c = (c00 * sx + c10 * tx) * sy + (c01 * sx + c11 * tx) * ty with c00 at
 *   (x, y), c10 at (x + 1, y), c01 at (x, y + 1) -- nfl_mesh_blend's expression.  The cell's origin ((k % cols) * C,
 *   (k / cols) * C) is added to the integers after the floor, never in floating point.
 *
 * NFL_EINVAL (nothing launched), all three: args NULL; a negative size, V > INT32_MAX or 3 T > INT32_MAX; cell outside
 *   [6, 1024], cols < 1, rows < 1, W * H > INT32_MAX, 2 * cols * rows < T; a NULL or misaligned (4 B) d_vertices /
 *   d_triangles (points: d_vertex_normals too) that a non-zero size needs.  points and resolve: a texel range that is negative
 *   or leaves the atlas; for n_texels > 0 a NULL or misaligned output (points) or d_sum (16 B) / d_views (resolve); a
 *   misaligned d_vertex_colors or d_texture.  nfl_mesh_shade_atlas: the table, run, n_vis, d_vis and alignment refusals of
 *   nfl_mesh_shade; both or neither of d_atlas and d_atlas_u8.  Zero texels or zero words: NFL_OK, no launch. */
typedef struct nfl_atlas_points_args {
    const float*   d_vertices;        /* (V, 3) world */
    const float*   d_vertex_normals;  /* (V, 3) */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    int32_t  cell, cols, rows, reserved;
    int64_t  first_texel, n_texels;
    float*   d_points;                /* out (n_texels, 3) */
    float*   d_normals;               /* out (n_texels, 3) */
} nfl_atlas_points_args;
int nfl_atlas_points(const nfl_atlas_points_args* args, void* stream);

typedef struct nfl_atlas_resolve_args {
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    int32_t  cell, cols, rows, reserved;
    int64_t  first_texel, n_texels;
    const float*   d_sum;             /* (n_texels, 4): nfl_mesh_blend over nfl_atlas_points' rows */
    const int32_t* d_views;           /* (n_texels) */
    const float*   d_vertex_colors;   /* (V, 3) or NULL: what an unseen texel interpolates */
    float    fallback[3];             /* an unseen texel without d_vertex_colors */
    float    background[3];           /* an ownerless texel */
    float*   d_texture;               /* out (n_texels, 3) or NULL */
    uint8_t* d_texture_u8;            /* out (n_texels, 3) or NULL */
    uint8_t* d_seen;                  /* out (n_texels) or NULL */
} nfl_atlas_resolve_args;
int nfl_atlas_resolve(const nfl_atlas_resolve_args* args, void* stream);

typedef struct nfl_mesh_shade_atlas_args {
    const float*   d_vertices;        /* (V, 3) world */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    const nfl_image_rec* d_table;     /* (n_images) */
    int32_t  n_images, first, count, reserved;
    const uint64_t* d_vis;            /* (n_vis): nfl_mesh_visibility of the same run */
    int64_t  n_vis;
    const float*   d_atlas;           /* (H, W, 3) fp32, or NULL */
    const uint8_t* d_atlas_u8;        /* (H, W, 3) bytes, or NULL: exactly one of the two */
    int32_t  cell, cols, rows, reserved2;
    float    background[3];
    int32_t  reserved3;
    float*   d_rgb;                   /* out (n_vis, 3) or NULL */
    uint8_t* d_rgb_u8;                /* out (n_vis, 3) or NULL */
    float*   d_depth;                 /* out (n_vis) or NULL */
    int32_t* d_triangle;              /* out (n_vis) or NULL */
} nfl_mesh_shade_atlas_args;
int nfl_mesh_shade_atlas(const nfl_mesh_shade_atlas_args* args, void* stream);

/* ---- depth fusion: depth maps of a run of cameras fused into a truncated signed distance function (TSDF) on a lattice, the
 * lattice points that were observed, and the vertices of a surface that stand on observed points only (the route NeRF
 * exporters take to a mesh: render a depth map per training camera, fuse, take the zero set) -----------------------------------
 * Every operation fp32 and rounded on its own, divisions and square roots correctly rounded; camera, run, q, dot and the
 * numbering of a run's depth words are those of "mesh colour" above, word for word, so a projection here has the bits of
 * nfl_mesh_blend's.  The lattice is nfl_surface's: (nz, ny, nx), x fastest, point (x, y, z) at p[k] = lo[k] + index[k] *
 * spacing[k], the product and the sum rounded separately.  A depth word is a distance from the camera centre, the unit of
 * nfl_mesh_depth and of depth_fine when |rays_d| = 1.  No memset, no copy, no allocation, no atomics, no scratch.
 *
 * nfl_tsdf_fuse   one launch, one thread per lattice point, the images of the run in increasing n inside.  For point p image
 *   n contributes when all of these hold:
 *     1  wi = d_image_weights[n] > 0 (NULL: 1 for every image; the array is indexed by the TABLE's n);
 *     2  s = -q.z > 0;
 *     3  u = cx + fx * (q.x / s), v = cy - fy * (q.y / s) with 0 <= u <= width - 1 and 0 <= v <= height - 1 (NaN fails);
 *     4  D = the depth word of pixel (floorf(u + 0.5f), floorf(v + 0.5f)), wp = its word of d_pixel_weights (NULL: 1),
 *        w = wi * wp, with w > 0 and D > 0 (NaN fails both; +inf passes: the ray hit nothing, so the point is free);
 *     5  e = t - p, dist = sqrt(dot(e, e)), phi = (dist - D) / trunc, and NOT phi > 1: a point more than trunc behind the
 *        surface is hidden, and nothing is known about it.  Then phi = fmaxf(phi, -1).
 *   The image adds w * phi to d_acc[p][0], w to d_acc[p][1] and 1 to d_views[p].  phi is positive BEHIND the surface: the
 *   inside of nfl_surface at iso = 0.  start != 0 begins the accumulators at zero, start == 0 continues what the caller's
 *   arrays hold, so a bank may be walked in runs; the result does not depend on the split.  A word outside [0, n_depth) is
 *   not read, and its image does not contribute.
 *   NFL_EINVAL (nothing launched): args / d_table NULL or d_table not 8-byte aligned, n_images < 1, a run outside the table,
 *   a size below 2 or above nfl_surface's limits (ny or nz above 65535, more than 2^30 points), trunc not positive or NaN,
 *   n_depth negative or above 2^38, d_depth NULL with n_depth > 0, d_acc or d_views NULL, a misaligned pointer (d_acc 8 B, the
 *   others 4 B).  count == 0 with start == 0: NFL_OK, no launch.
 *
 * nfl_tsdf_resolve   one launch, one thread per lattice point: where d_acc[p][1] >= min_weight and d_views[p] >= min_views,
 *   d_lattice[p] = d_acc[p][0] / d_acc[p][1] and d_known[p] = 1; elsewhere d_lattice[p] = fill and d_known[p] = 0.
 *   NFL_EINVAL: args or one of the four arrays NULL or misaligned, the sizes as above, min_weight not positive or NaN,
 *   min_views < 1, a NaN fill.
 *
 * nfl_tsdf_support   one launch, one thread per vertex: g[k] = (p[k] - lo[k]) / spacing[k]; the vertex is unsupported when
 *   any g[k] is not finite or lies outside [0, n[k] - 1]; otherwise a[k] = floorf(g[k]), b[k] = ceilf(g[k]) and d_support[v] = 1
 *   when d_known holds at every lattice point of {a.x, b.x} x {a.y, b.y} x {a.z, b.z}, else 0.  A vertex of nfl_surface lies on
 *   a lattice edge: on an axis edge the rule reads "both ends of the crossing edge were observed", on a diagonal its face or
 *   its cell.  nfl_surface counts the fill value of an unobserved point as outside, so without this rule a fused lattice
 *   grows a second wall where the observed band behind the surface ends.
 *   NFL_EINVAL: args or d_known NULL, the sizes as above, V < 0 or above INT32_MAX, and for V > 0 a NULL d_vertices / d_support
 *   or a misaligned d_vertices.  V == 0: NFL_OK, no launch. */
typedef struct nfl_tsdf_fuse_args {
    const nfl_image_rec* d_table;     /* (n_images) */
    int32_t  n_images, first, count;
    int32_t  start;                   /* != 0: the accumulators begin at zero */
    const float* d_depth;             /* (n_depth): the run's depth words, nfl_mesh_depth's numbering */
    int64_t  n_depth;
    const float* d_pixel_weights;     /* (n_depth) or NULL */
    const float* d_image_weights;     /* (n_images) or NULL */
    int32_t  nx, ny, nz;
    float    trunc;
    float    lo[3];                   /* position of lattice point (0, 0, 0): x, y, z */
    float    spacing[3];              /* x, y, z */
    float*   d_acc;                   /* in/out (nz, ny, nx, 2): sum of w * phi, sum of w */
    int32_t* d_views;                 /* in/out (nz, ny, nx) */
} nfl_tsdf_fuse_args;
int nfl_tsdf_fuse(const nfl_tsdf_fuse_args* args, void* stream);

typedef struct nfl_tsdf_resolve_args {
    const float*   d_acc;             /* (nz, ny, nx, 2) */
    const int32_t* d_views;           /* (nz, ny, nx) */
    int32_t  nx, ny, nz, min_views;
    float    min_weight, fill;
    float*   d_lattice;               /* out (nz, ny, nx) */
    uint8_t* d_known;                 /* out (nz, ny, nx) */
} nfl_tsdf_resolve_args;
int nfl_tsdf_resolve(const nfl_tsdf_resolve_args* args, void* stream);

typedef struct nfl_tsdf_support_args {
    const float*   d_vertices;        /* (V, 3) */
    int64_t  n_vertices;
    const uint8_t* d_known;           /* (nz, ny, nx) */
    int32_t  nx, ny, nz, reserved;
    float    lo[3];
    float    spacing[3];
    uint8_t* d_support;               /* out (V) */
} nfl_tsdf_support_args;
int nfl_tsdf_support(const nfl_tsdf_support_args* args, void* stream);

/* ---- mesh distance: the closest point of a triangle mesh for many query points, a uniform grid of triangle lists that finds it
 * without trying every triangle, area-weighted samples of a surface, and the reduction of a run of distances (what Chamfer
 * distance, Hausdorff distance and the F-score of a reconstruction are made of) --------------------------------------------------
 * Every operation fp32 and rounded on its own unless fp64 is named, divisions and square roots correctly rounded; dot and cross
 * are those of "mesh colour" above.  Triangle indices are NOT trusted.  A triangle is USABLE when its three indices lie in
 * [0, n_vertices) and its nine coordinates are finite; every other triangle is listed nowhere, is never an answer and gets
 * no sample.  mix(x) is the finaliser of splitmix64 on uint64 (x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27,
 * x *= 0x94D049BB133111EB, x ^= x >> 31), sums of uint64 wrap.
 *
 * THE GRID is lo[3], one cell size `cell` (cubic cells) and dims[3] = (nx, ny, nz) cells, 1 <= dims[k] <= 65535 and at most
 * 2^30 cells; cell (x, y, z) is number (z * ny + y) * nx + x.  The cell of a coordinate on axis k is
 *     cellf(x) = (int)fminf(fmaxf(floorf((x - lo[k]) / cell), 0), (float)(dims[k] - 1)),
 * a monotone function of x (a NaN goes to cell 0).  A usable triangle is listed in every cell of the index box
 * [cellf(min corner), cellf(max corner)] of its bounding box, so by monotonicity every point of it lies in a cell that lists
 * it (after clamping, too: the cells on the grid's faces list what lies beyond them).
 *
 * nfl_trigrid_count   zero, one thread per triangle (an int32 atomicAdd per cell of its box), a scan of the counts to int64.
 *   d_totals[0] = the entries of all rows, d_totals[1] = the triangles with an index outside [0, n_vertices).
 * nfl_trigrid_emit    d_offsets (cells + 1) int64, row c being d_entries[d_offsets[c] .. d_offsets[c + 1]), and the rows,
 *   filled through a per-cell cursor: the ORDER INSIDE A ROW IS NOT DEFINED, and nothing below depends on it.
 *   n_entries = d_totals[0] of the count call on the same scratch; at most INT32_MAX.
 *   NFL_EINVAL (nothing launched), both: args NULL, a negative size, V > INT32_MAX or 3 T > INT32_MAX, dims as above, cell not
 *   positive or not finite, a non-finite lo, a NULL or misaligned (4 B) d_vertices / d_triangles that a non-zero size needs,
 *   d_totals NULL (count), n_entries negative or above INT32_MAX or a NULL / misaligned d_offsets (8 B) / d_entries (emit).
 *   The scratch as everywhere: NULL or misaligned NFL_EINVAL, short NFL_ESMALL.  T == 0 is served: empty rows.
 *
 * POINT AND TRIANGLE.  For a query p and a usable triangle (a, b, c), the seven regions of Ericson, Real-Time Collision
 * Detection, 5.1.5.  THIS PARAGRAPH IS FP64, every operation rounded on its own, the fp32 inputs converted first (the 2 x 2
 * determinants below cancel: in fp32 the slivers that marching tetrahedra leave put q some 3e-6 away from a point that lay
 * on the triangle): ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap); bp = p - b, d3 = dot(ab, bp),
 * d4 = dot(ac, bp); cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp); vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6,
 * va = d3 * d6 - d5 * d4.  The first of these that holds gives the barycentrics (u, v, w) of a, b, c and the point q, each
 * rounded to fp32 at the end:
 *     1  d1 <= 0 and d2 <= 0                          (1, 0, 0), q = a
 *     2  d3 >= 0 and d4 <= d3                         (0, 1, 0), q = b
 *     3  vc <= 0 and d1 >= 0 and d3 <= 0              s = d1 / (d1 - d3): (1 - s, s, 0), q = a + s * ab
 *     4  d6 >= 0 and d5 <= d6                         (0, 0, 1), q = c
 *     5  vb <= 0 and d2 >= 0 and d6 <= 0              s = d2 / (d2 - d6): (1 - s, 0, s), q = a + s * ac
 *     6  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    s = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (0, 1 - s, s), q = b + s * (c - b)
 *     7  otherwise                                    den = 1 / ((va + vb) + vc), s = vb * den, r = vc * den:
 *                                                     ((1 - s) - r, s, r), q = (a + s * ab) + r * ac.
 * Back in fp32, q is CLAMPED into the triangle's bounding box, q[k] = mn[k] when q[k] < mn[k], mx[k] when q[k] > mx[k], else
 * q[k] (a NaN stays), mn and mx the least and the largest of the three corners -- rounding moves q out by an ulp at most,
 * and the clamp is what the grid's stopping rule stands on -- and with e = p - q, dd = (e0 * e0 + e1 * e1) + e2 * e2.  A candidate is ACCEPTED when dd <= max_distance * max_distance and dd < +inf (a NaN,
 * which a degenerate triangle can give through 0 / 0, fails).  The answer is the accepted candidate with the least
 * (dd, triangle index): ties go to the lower index, so the answer depends neither on the order in which triangles are tried
 * nor on how often.
 *
 * nfl_mesh_closest   one launch, one thread per query.  d_distance = sqrtf(dd), d_triangle, d_point = q, d_bary = (u, v, w)
 *   of the answer; with d_normals (a vector per query) and d_dot, d_dot = dot(query vector, face normal), the face normal
 *   cross(ab, ac) divided by its length sqrtf(dot(cr, cr)), three zeros when that length is zero.  A query with no accepted
 *   candidate -- nothing within max_distance, an empty mesh, a non-finite query coordinate -- gets +inf, -1 and NaNs.
 *   max_distance is positive; +inf means no limit.
 *   BRUTE (d_offsets NULL): every query tries every triangle, which a workgroup stages through LDS 256 at a time.
 *   GRID (d_offsets, d_entries, n_entries, lo, cell, dims of nfl_trigrid_emit for the SAME mesh): with C the query's own cell
 *   (cellf per axis), shells r = 0, 1, 2, ...: shell r is the cells at Chebyshev distance r from C inside the grid, and every
 *   triangle its rows list is tried.  After shell r the block [C - r, C + r], cut to the grid, has been walked; a usable
 *   triangle NOT listed in it lies, on some axis k, wholly beyond a face of the block that is not a face of the grid.  The
 *   walk ends when the block is the whole grid, or when best < bound or bound > max_distance^2, best being the least accepted
 *   dd so far (+inf: none) and bound the minimum over the block's faces that are not faces of the grid of g * g, where
 *   g = (float)(G * (1 - 2^-23)) and, in FP64, with F = lo[k] + i * cell the face at index i (i = the block's first index, or
 *   its last + 1) and S = 2^-21 * (|lo[k]| + i * cell):  G = p[k] - (F + S) on the low side, (F - S) - p[k] on the high side,
 *   0 when that is negative.  The slack S is explicit because cellf is computed in fp32: the smallest x with cellf(x) >= i
 *   lies within S of F.  Every corner of an unlisted triangle beyond that face, hence (the clamp) its q[k], is then at least
 *   G from p[k]; fp32 rounding is monotone, so |e[k]| >= g and dd >= g * g = bound > best: it can neither win nor tie.
 *   THE CONTRACT: grid mode returns the bits of brute mode, for every cell size and every origin.
 *   A grid that is not this mesh's (rows out of range, unknown triangles) is read inside its arrays and never faults.
 *   NFL_EINVAL (nothing launched): args NULL, a negative size, the mesh sizes as above, max_distance not positive (NaN
 *   included), and for N > 0 a NULL or misaligned (4 B) d_points or output, d_normals without d_dot or the reverse; in grid
 *   mode dims / cell / lo as above, d_entries NULL with n_entries > 0, n_entries outside [0, INT32_MAX], d_offsets not 8-byte
 *   aligned.  N == 0: NFL_OK, no launch.
 *
 * SURFACE SAMPLES.  For triangle t: cr = cross(b - a, c - a), len = sqrtf(dot(cr, cr)), area = 0.5f * len;
 *   ht = mix(mix(seed) + t), ut = (float)(ht >> 40) * 2^-24 (24 bits, in [0, 1)), m_t = floorf(area * density + ut): the
 *   rounding is stochastic, so the expected count is area * density exactly and small triangles are not starved.  A triangle
 *   that is not usable, or whose len is zero or not finite, has m_t = 0.  Sample j of triangle t: hj = mix(ht + (j + 1)),
 *   k1 = hj >> 40, k2 = (hj >> 16) & 0xFFFFFF, r = ((float)k + 0.5f) * 2^-24 each (in (0, 1]; the sum rounds to even above
 *   2^23); when r1 + r2 > 1 both become 1 - r; p = (a + r1 * (b - a)) + r2 * (c - a); the normal is cr[k] / len.
 *   Samples lie in triangle order, sample j of triangle t at row (the m of the triangles before t) + j.
 * nfl_mesh_sample_count   d_totals[0] = the samples, [1] = triangles with an index out of range, [2] = triangles whose
 *   area * density + ut is 2^24 or more (they count 0; the caller refuses).
 * nfl_mesh_sample_emit    d_points (n_samples, 3), d_sample_triangles (n_samples) int32, d_normals (n_samples, 3).  A triangle
 *   of more than 64 samples is written by its whole wave, in the same launch.  n_samples = d_totals[0], at most INT32_MAX.
 *   NFL_EINVAL: args NULL, the mesh sizes and pointers as above, density negative or not finite, d_totals NULL (count),
 *   n_samples outside [0, INT32_MAX] or a NULL / misaligned output with n_samples > 0 (emit); the scratch as everywhere.
 *
 * nfl_meshdist_reduce   two launches, no atomics: d_row (NFL_MESHDIST_COLUMNS fp64) of n distances.  An element COUNTS when
 *   its distance d is below +inf (a NaN does not count; +inf is what max_distance leaves).  Columns: the count; the sum of d;
 *   of d * d (in fp64); the maximum of d (0 when nothing counts); for k < n_tau the count of d <= tau[k] (fp32 comparison),
 *   0 for k >= n_tau; the sum of |d_dot| over the counting elements (0 without d_dot).  G = min(ceil(n / 256), 1024) workgroups
 *   of 256: thread t of workgroup g adds elements (g + j * G) * 256 + t, j = 0, 1, ... in that order in fp64, the 256 threads
 *   are folded by halving (row t += row t + off for t < off, off = 128 .. 1), the G partial rows are dealt to the 256
 *   threads of ONE workgroup (thread t adds rows t, t + 256, ... in order) and folded the same way; maxima by fmax.  The row
 *   is bit-reproducible.
 *   NFL_EINVAL: args, d_distance (n > 0) or d_row NULL, misaligned pointers (4 B; d_row and the scratch 8 B), n negative or
 *   above INT32_MAX, n_tau outside [0, 8], a NaN tau below n_tau.  n == 0 writes the row of zeros. */
#define NFL_MESHDIST_MAX_TAU 8
enum { NFL_MESHDIST_COUNT = 0, NFL_MESHDIST_SUM = 1, NFL_MESHDIST_SUM_SQ = 2, NFL_MESHDIST_MAX = 3, NFL_MESHDIST_WITHIN = 4,
       NFL_MESHDIST_SUM_DOT = 12, NFL_MESHDIST_COLUMNS = 13 };
typedef struct nfl_trigrid_args {
    const float*   d_vertices;        /* (V, 3) */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    float    lo[3];
    float    cell;
    int32_t  dims[3];                 /* cells along x, y, z */
    int32_t  reserved;
    void*    d_scratch;               /* nfl_trigrid_bytes(dims); the emit call reads what the count call left */
    size_t   scratch_bytes;
    int64_t* d_totals;                /* count: out (2) */
    int64_t  n_entries;               /* emit: d_totals[0] */
    int64_t* d_offsets;               /* emit: out (cells + 1) */
    int32_t* d_entries;               /* emit: out (n_entries) */
} nfl_trigrid_args;
size_t nfl_trigrid_bytes(int32_t nx, int32_t ny, int32_t nz);
int nfl_trigrid_count(const nfl_trigrid_args* args, void* stream);
int nfl_trigrid_emit(const nfl_trigrid_args* args, void* stream);

typedef struct nfl_mesh_closest_args {
    const float*   d_points;          /* (N, 3) queries */
    int64_t  n_points;
    const float*   d_vertices;        /* (V, 3) */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    const int64_t* d_offsets;         /* (cells + 1) of nfl_trigrid_emit, or NULL: brute mode */
    const int32_t* d_entries;         /* (n_entries) */
    int64_t  n_entries;
    float    lo[3];
    float    cell;
    int32_t  dims[3];
    float    max_distance;            /* positive; +inf: no limit */
    const float*   d_normals;         /* (N, 3) a vector per query, or NULL */
    float*   d_distance;              /* out (N) */
    int32_t* d_triangle;              /* out (N) */
    float*   d_point;                 /* out (N, 3) */
    float*   d_bary;                  /* out (N, 3) */
    float*   d_dot;                   /* out (N), with d_normals; else NULL */
} nfl_mesh_closest_args;
int nfl_mesh_closest(const nfl_mesh_closest_args* args, void* stream);

typedef struct nfl_mesh_sample_args {
    const float*   d_vertices;        /* (V, 3) */
    const int32_t* d_triangles;       /* (T, 3) */
    int64_t  n_vertices, n_triangles;
    uint64_t seed;
    float    density;                 /* samples per unit area */
    int32_t  reserved;
    void*    d_scratch;               /* nfl_mesh_sample_bytes(T) */
    size_t   scratch_bytes;
    int64_t* d_totals;                /* count: out (3) */
    int64_t  n_samples;               /* emit: d_totals[0] */
    float*   d_points;                /* emit: out (n_samples, 3) */
    int32_t* d_sample_triangles;      /* emit: out (n_samples) */
    float*   d_normals;               /* emit: out (n_samples, 3) */
} nfl_mesh_sample_args;
size_t nfl_mesh_sample_bytes(int64_t n_triangles);
int nfl_mesh_sample_count(const nfl_mesh_sample_args* args, void* stream);
int nfl_mesh_sample_emit(const nfl_mesh_sample_args* args, void* stream);

typedef struct nfl_meshdist_reduce_args {
    const float* d_distance;          /* (n) */
    const float* d_dot;               /* (n) or NULL */
    int64_t  n;
    int32_t  n_tau;
    float    tau[NFL_MESHDIST_MAX_TAU];
    int32_t  reserved;
    void*    d_scratch;               /* nfl_meshdist_reduce_bytes(n) */
    size_t   scratch_bytes;
    double*  d_row;                   /* out (NFL_MESHDIST_COLUMNS) */
} nfl_meshdist_reduce_args;
size_t nfl_meshdist_reduce_bytes(int64_t n);
int nfl_meshdist_reduce(const nfl_meshdist_reduce_args* args, void* stream);

/* ---- registration: the similarity transform x' = s R x + t that brings points onto a mesh (point-to-plane or point-to-point
 * ICP around nfl_mesh_closest) or onto given partners (the closed form) -------------------------------------------------------
 * Entry points take pointers and scalars; there is no argument struct.  EVERYTHING HERE IS FP64 unless fp32 is named, every
 * operation rounded on its own, divisions and square roots correctly rounded, sums of three written (x + y) + z, the fp32
 * inputs converted first.  A TRANSFORM is NFL_REGISTER_TRANSFORM = 13 doubles in device memory: s, R row-major (9), t (3).
 *
 * nfl_register_apply   one thread per row of d_in (n, 3) fp32: y_i = (R_i0 x_0 + R_i1 x_1) + R_i2 x_2, and
 *   d_out_i = (float)(s * y_i + t_i), with vectors = 1 (float)y_i (normals: rotated only).  The transform is read from device
 *   memory by the kernel; d_in == d_out is allowed.
 *
 * nfl_register_moments   the row d_row (NFL_REGISTER_COLUMNS) of n pairs: P = d_points (the transformed points), Q = d_closest,
 *   and d_triangle, d_distance as nfl_mesh_closest left them for P.  A pair COUNTS when the six coordinates of P and Q are
 *   finite, its distance d is below +inf and d <= max_distance (fp32 comparison; +inf: no limit), and its triangle index t lies
 *   in [0, n_triangles), is USABLE in the sense of "mesh distance" and has a face normal: with ab, ac, cr = cross(ab, ac) and
 *   len = sqrtf(dot(cr, cr)) IN FP32 as nfl_mesh_closest computes them for d_dot, 0 < len < +inf, and nf = cr / len.  In point
 *   mode d_distance and d_triangle may each be NULL: that test is then not made (given partners).
 *   With c = (cx, cy, cz), p = P - c, q = Q - c, e = P - Q:
 *     NFL_REGISTER_COUNT   1 per counting pair          NFL_REGISTER_SUM_DD   d * d; without d_distance (e0 e0 + e1 e1) + e2 e2
 *   NFL_REGISTER_POINT:  SUM_P + k = p_k, SUM_Q + k = q_k, SUM_PP = (p0 p0 + p1 p1) + p2 p2, SUM_QQ likewise,
 *     SUM_PQ + 3 i + j = p_i q_j.
 *   NFL_REGISTER_PLANE:  N = nf; a = (p x N, N, N . p), a 7-vector: a0 = p1 N2 - p2 N1, a1 = p2 N0 - p0 N2,
 *     a2 = p0 N1 - p1 N0, a6 = (p0 N0 + p1 N1) + p2 N2; r = (N0 e0 + N1 e1) + N2 e2.  ATA + (the place of (i, j), i <= j, in
 *     the upper triangle read row by row: 7 i - i (i - 1) / 2 + j - i) = a_i a_j; ATB + i = a_i r; SUM_RR = r r.
 *   The columns of the other mode are zeros.  The order of the additions is nfl_meshdist_reduce's: G = min(ceil(n / 256), 1024)
 *   workgroups of 256, thread t of workgroup g adds elements (g + j G) * 256 + t, j = 0, 1, ... in order (a pair that does not
 *   count adds nothing), the 256 threads are folded by halving, the G partial rows are dealt to the 256 threads of ONE
 *   workgroup (thread t adds rows t, t + 256, ...) and folded the same way.  No float atomics: the row is bit-reproducible.
 *   The scratch is nfl_register_bytes(n): a partial row per workgroup.  n == 0 writes the row of zeros.
 *
 * nfl_register_solve   one working thread.  From the row an increment (ds, dR, dt), composed IN PLACE into d_transform:
 *   s <- ds s;  R <- dR R (R_ij = (dR_i0 R_0j + dR_i1 R_1j) + dR_i2 R_2j);  t <- ds (dR t) + dt, dR t as y above.
 *   d_history[4 iteration ..] = (count, sqrt(SUM_DD / count), status, the s that is left).  Status: NFL_REGISTER_OK;
 *   NFL_REGISTER_FEW when count < min_pairs; NFL_REGISTER_SINGULAR when a pivot below is not > 0 (a NaN is not) or one of the
 *   13 new doubles is not finite.  On either failure the transform is left as it was, bit for bit.
 *   rot(w, x, y, z) of a unit quaternion, by products: R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), R02 = 2 (xz + wy),
 *   R10 = 2 (xy + wz), R11 = 1 - 2 (xx + zz), R12 = 2 (yz - wx), R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = 1 - 2 (xx + yy).
 *   POINT (Horn 1987; Umeyama's problem): n = count, mp = SUM_P / n, mq = SUM_Q / n, M_ij = SUM_PQ_ij - SUM_P_i * mq_j;
 *     N = the symmetric 4 x 4 matrix  [ (M00 + M11) + M22,  M12 - M21,          M20 - M02,          M01 - M10
 *                                                         (M00 - M11) - M22,  M01 + M10,          M20 + M02
 *                                                                             (M11 - M00) - M22,  M12 + M21
 *                                                                                                 (M22 - M00) - M11 ];
 *     V = I; 12 sweeps of cyclic Jacobi over (p, q) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3); a rotation whose A_pq is
 *     exactly 0 is skipped; g = A_pq, theta = (A_qq - A_pp) / (2 g), t = sgn / (|theta| + sqrt(theta theta + 1)) with
 *     sgn = 1 for theta >= 0, else -1; c = 1 / sqrt(t t + 1), s = t c; A_pp -= t g, A_qq += t g, A_pq = A_qp = 0; for the
 *     two other r:  (A_rp, A_rq) <- (c A_rp - s A_rq, s A_rp + c A_rq), mirrored; for all r the same of (V_rp, V_rq).
 *     The column of V under the largest diagonal entry (the lowest index on a tie) is (w, x, y, z) after scaling by
 *     1 / sqrt(((v0 v0 + v1 v1) + v2 v2) + v3 v3) and negating all four when w < 0.  dR = rot(w, x, y, z).
 *     With scale, the pivot is den = SUM_PP - ((SUM_P0 mp0 + SUM_P1 mp1) + SUM_P2 mp2) and ds = (sum over i = 0..2, then
 *     j = 0..2, added one after the other to 0, of dR_ij M_ji) / den; a ds that is not > 0 is SINGULAR; without, ds = 1.
 *     dt_i = (mq_i + c_i) - ds * y_i, y = dR (mp + c).
 *   PLANE: the leading m x m system, m = 7 with scale and 6 without, A x = -b by Cholesky A = L L^T: for j = 0 .. m - 1:
 *     d = A_jj, then d -= L_jk L_jk for k = 0 .. j - 1, the pivot d, L_jj = sqrt(d); for i > j: v = A_ji, v -= L_ik L_jk
 *     for k < j, L_ij = v / L_jj.  Forward: y_i = (-b_i - L_i0 y_0 - ... - L_i,i-1 y_i-1) / L_ii in that order; backward from
 *     i = m - 1: x_i = (y_i - L_i+1,i x_i+1 - ... - L_m-1,i x_m-1) / L_ii, k ascending.
 *     (h0, h1, h2) = 0.5 * x[0..2], k = 1 / sqrt(((1 + h0 h0) + h1 h1) + h2 h2), dR = rot(k, h0 k, h1 k, h2 k) -- a
 *     rotation about x[0..2] by 2 atan(|x[0..2]| / 2), rational but for one square root; ds = 1 + x[6] with scale (not > 0:
 *     SINGULAR), else 1; dt_i = (c_i + x[3 + i]) - ds * y_i, y = dR c.
 *
 *   NFL_EINVAL (nothing launched): n negative or above INT32_MAX, the mesh sizes as in "mesh distance", a mode outside the
 *   enum, vectors / with_scale outside {0, 1}, max_distance not positive (NaN included), a non-finite cx, cy or cz,
 *   min_pairs < 1, iteration negative or above INT32_MAX / 4; d_transform, d_row or d_history NULL or not 8-byte aligned; for
 *   n > 0 a NULL or misaligned (4 B) d_in, d_out, d_points or d_closest, in plane mode also d_triangle and d_distance, and
 *   wherever d_triangle is given the mesh pointers a non-zero size needs.  The scratch as everywhere: NULL or misaligned
 *   NFL_EINVAL, short NFL_ESMALL.  nfl_register_apply with n == 0: NFL_OK, no launch.  nfl_register_bytes: 0 for such an n. */
enum { NFL_REGISTER_POINT = 0, NFL_REGISTER_PLANE = 1 };
enum { NFL_REGISTER_OK = 0, NFL_REGISTER_FEW = 1, NFL_REGISTER_SINGULAR = 2 };
#define NFL_REGISTER_TRANSFORM 13
#define NFL_REGISTER_HISTORY 4
enum { NFL_REGISTER_COUNT = 0, NFL_REGISTER_SUM_DD = 1, NFL_REGISTER_SUM_P = 2, NFL_REGISTER_SUM_Q = 5, NFL_REGISTER_SUM_PP = 8,
       NFL_REGISTER_SUM_QQ = 9, NFL_REGISTER_SUM_PQ = 10, NFL_REGISTER_ATA = 19, NFL_REGISTER_ATB = 47, NFL_REGISTER_SUM_RR = 54,
       NFL_REGISTER_COLUMNS = 55 };
size_t nfl_register_bytes(int64_t n);
int nfl_register_apply(const float* d_in, float* d_out, int64_t n, const double* d_transform, int32_t vectors, void* stream);
int nfl_register_moments(const float* d_points, const float* d_closest, const int32_t* d_triangle, const float* d_distance,
                         const float* d_vertices, const int32_t* d_triangles, int64_t n, int64_t n_vertices, int64_t n_triangles,
                         int32_t mode, float max_distance, double cx, double cy, double cz,
                         void* d_scratch, size_t scratch_bytes, double* d_row, void* stream);
int nfl_register_solve(const double* d_row, int32_t mode, int32_t with_scale, int64_t min_pairs, double cx, double cy, double cz,
                       double* d_transform, double* d_history, int32_t iteration, void* stream);

/* ---- mesh cast: where an arbitrary ray first hits a triangle mesh, whether it hits it at all, and the share of a point's
 * hemisphere that the mesh leaves open (ambient occlusion); through THE GRID of "mesh distance", or trying every triangle --------
 * Entry points take pointers and scalars; there is no argument struct.  Triangles are USABLE in the sense of "mesh distance",
 * every other triangle is never hit; mix() is that section's.  A RAY is 8 floats [o (3), d (3), near, far]; d need not be
 * normalised, t is the ray's own parameter.  A ray with a non-finite o or d, a NaN near or far, d == 0 or near > far hits
 * nothing; near = -inf and far = +inf are allowed.
 *
 * THE RAY TEST of a ray and a usable triangle (a, b, c).  THIS PARAGRAPH IS FP64, every operation rounded on its own, the fp32
 * inputs converted first, dot(x, y) = (x0 y0 + x1 y1) + x2 y2, cross(x, y) = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0):
 *   e1 = b - a, e2 = c - a, p = cross(d, e2), det = dot(e1, p); a det that is 0 or NaN is a miss (both faces hit: no culling);
 *   s = o - a, u = dot(s, p) / det, q = cross(s, e1), v = dot(d, q) / det, t = dot(e2, q) / det.
 *   The hit needs u >= 0, v >= 0, u + v <= 1, and tf = (float)t finite with near <= tf <= far (fp32 comparisons).
 *   Q = (a + u * e1) + v * e2; qf[k] = (float)Q[k] CLAMPED into the triangle's fp32 bounding box as "mesh distance" clamps q.
 *   THE CONSISTENCY CONDITION: with td[k] = t * d[k], on every axis |(o[k] + td[k]) - qf[k]| <= tol, where
 *   tol = 2^-20 * max over k of (|o[k]| + |td[k]|).  It fails only where the conditioning of the test is beyond about 1e10
 *   (triangles seen edge-on), and it is what the grid walk stands on: an accepted hit lies within tol of the ray, and (the
 *   clamp, cellf being monotone) in a cell that lists its triangle.
 *   THE BOX RULE, wherever a grid is given (lo, cell, dims; with or without its rows): on every axis
 *   lo[k] <= qf[k] <= lo[k] + dims[k] * cell, the right side in fp64.  Space outside the grid's box is empty, as in "occupancy".
 *   The hit carries tf, the corner weights ((float)((1 - u) - v), (float)u, (float)v) of a, b, c, and qf.
 * THE ANSWER of a ray is the accepted hit with the least (tf, triangle index): ties go to the lower index, so the answer
 * depends neither on the order in which triangles are tried nor on how often.
 *
 * THE WALK (grid mode), in fp64.  m = the axis of the largest |d[k]|, the lowest on a tie.  E = 2^-19 * (2 * max|o[k]| + bmax),
 * bmax the largest absolute coordinate of the box's two corners: inside the box tol <= E / 2 for every accepted hit, whatever
 * its t.  tn = near - (|near| * 2^-23 + 2^-148), tf' = far + (|far| * 2^-23 + 2^-148): every t with near <= (float)t <= far
 * lies in [tn, tf'].  Slab i of axis m is the cells with index i there; with F, S the faces and slacks of "mesh distance", a hit
 * whose qf[m] has cellf = i has o[m] + t * d[m] in [(F_i - S_i) - E, (F_i+1 + S_i+1) + E]; dividing the ends by d[m] gives
 * [te_i, tx_i], and te_i does not decrease along the walk.  The slabs are taken in the ray's direction from two slabs before
 * the one that floor() puts o[m] + tn * d[m] - (E + S) in; a slab with tx_i < tn is passed over; the walk ends at te_i > tf',
 * at the grid's last slab, or BEFORE slab i when a hit is held whose tf is STRICTLY below (te_i - |te_i| * 2^-40) rounded down
 * to fp32.  In a slab, on each other axis k the coordinates o[k] + t * d[k] at the two ends of [max(te, tn), min(tx, tf')],
 * the lesser minus E rounded down to fp32, the greater plus E rounded up, go through cellf: every triangle of every row of
 * that block of cells (at most 3 x 3 when E is small beside a cell, |d[k]| <= |d[m]|) is tried with THE RAY TEST.  Any-hit
 * mode ends at the first accepted hit.  THE CONTRACT: grid mode returns the bits of brute mode given the same box, for every
 * cell size and every origin.  A grid that is not this mesh's is read inside its arrays and never faults.
 *
 * nfl_mesh_cast   one launch, one thread per ray of d_rays (n_rays, 8).  BRUTE (d_offsets NULL): every ray tries every triangle,
 *   staged through LDS 256 at a time; with nx = ny = nz = 0 there is no box rule, otherwise lo, cell and dims give the box.
 *   GRID: d_offsets, d_entries, n_entries, lo, cell, dims of nfl_trigrid_emit for the SAME mesh.  NFL_CAST_FIRST writes d_t = tf
 *   (+inf on a miss) and, where given, d_triangle (-1), d_bary (n_rays, 3) and d_point (n_rays, 3) = qf (NaN on a miss);
 *   NFL_CAST_ANY writes d_t alone: 0 for a ray that hits anything, +inf for one that does not.
 * nfl_mesh_occlusion   one launch, a wave per point i of d_points with normal n = d_normals[i] (unit length is the caller's):
 *   the origin is o[k] = p[k] + bias * n[k] (fp32).  DIRECTION j < n_directions, fp32 throughout, no trigonometry:
 *   h = mix(mix(mix(seed) + i) + j); attempt a = 0 .. 7: ha = mix(h + (a + 1)), x = (float)(ha >> 40) * 2^-23 - 1,
 *   y = (float)((ha >> 16) & 0xFFFFFF) * 2^-23 - 1 (both exact, in [-1, 1)), s = x * x + y * y; the first attempt with s < 1
 *   is taken, (x, y, s) = (0, 0, 0) if there is none; z = sqrtf(1 - s).  The frame (Duff et al. 2017): sg = copysignf(1, n2),
 *   A = -1 / (sg + n2), B = (n0 * n1) * A, t1 = (1 + ((sg * n0) * n0) * A, sg * B, -(sg * n0)), t2 = (B, sg + (n1 * n1) * A, -n1);
 *   d[k] = (x * t1[k] + y * t2[k]) + z * n[k]: cosine-weighted about n.  The ray [0, radius] is walked in any-hit mode;
 *   d_hits[i] = the rays that hit (counted by ballot: no order enters), d_open[i] = (float)(n_directions - hits) / (float)
 *   n_directions.  A point or normal with a non-finite coordinate, or a zero normal: d_hits = -1, d_open = NaN.  The grid is
 *   required.  radius = +inf means no limit inside the box.
 *
 *   NFL_EINVAL (nothing launched): n_rays / n negative or above INT32_MAX, the mesh sizes and pointers as in "mesh distance",
 *   a mode outside the enum, n_directions outside [1, 4096], radius not positive (NaN included), bias negative or not finite;
 *   with d_offsets: dims / cell / lo as in "mesh distance", d_entries NULL or misaligned with n_entries > 0, n_entries outside
 *   [0, INT32_MAX], d_offsets not 8-byte aligned; without (nfl_mesh_cast only; nfl_mesh_occlusion refuses): dims neither all
 *   zero nor a grid's; for n > 0 a NULL or misaligned (4 B) d_rays, d_t, d_points, d_normals, d_hits or d_open, a misaligned
 *   optional output.  n == 0: NFL_OK, no launch. */
enum { NFL_CAST_FIRST = 0, NFL_CAST_ANY = 1 };
int nfl_mesh_cast(const float* d_rays, int64_t n_rays, const float* d_vertices, const int32_t* d_triangles, int64_t n_vertices,
                  int64_t n_triangles, const int64_t* d_offsets, const int32_t* d_entries, int64_t n_entries,
                  float lo_x, float lo_y, float lo_z, float cell, int32_t nx, int32_t ny, int32_t nz, int32_t mode,
                  float* d_t, int32_t* d_triangle, float* d_bary, float* d_point, void* stream);
int nfl_mesh_occlusion(const float* d_points, const float* d_normals, int64_t n, const float* d_vertices,
                       const int32_t* d_triangles, int64_t n_vertices, int64_t n_triangles, const int64_t* d_offsets,
                       const int32_t* d_entries, int64_t n_entries, float lo_x, float lo_y, float lo_z, float cell,
                       int32_t nx, int32_t ny, int32_t nz, int32_t n_directions, float radius, float bias, uint64_t seed,
                       int32_t* d_hits, float* d_open, void* stream);

/* ---- mesh solid: how often a ray crosses a mesh, and from that whether a point lies inside a closed one ----------------------
 * Everything here stands on "mesh cast": the rays, the usable triangles, THE RAY TEST with its clamp, its consistency condition
 * and its box rule, THE WALK.  Nothing of them changes.
 *
 * THE CROSSINGS of a ray: the number of usable triangles whose RAY TEST accepts the ray (with the box rule wherever a grid or a
 * box is given).  A ray that can hit nothing counts 0; far = +inf is served.  Every triangle counts at most once; a triangle
 * that the mesh holds twice is two triangles.
 * THE ONCE-ONLY RULE (grid mode).  THE WALK is run to its end -- there is no held hit, so it ends at te_i > tf' or at the grid's
 * last slab only -- and reads a triangle in every cell of its bounding box that it passes.  An accepted hit counts only in
 * the cell (cellf(qf[0]), cellf(qf[1]), cellf(qf[2])) of its own clamped point qf.  That cell lists the triangle (the clamp
 * keeps qf in its bounding box), it is read while slab cellf(qf[m]) is walked ("mesh cast": the hit's parameter lies in that
 * slab's interval, and on the two other axes qf lies within E of the ray there), and no cell is read twice, the slabs being
 * taken in order.  THE CONTRACT: grid mode returns the integer of brute mode given the same box.
 *
 * THE DIRECTIONS: 7 fixed fp32 vectors, NFL_SOLID_DIRECTIONS below, component k of direction j being sign * sqrt(prime) rounded
 * to fp32, 21 distinct primes: no component is zero, none runs along a lattice line or in a face of an axis-aligned box, the
 * major axes go x, y, z, x, y, z, x and the signs differ.  They are not normalised.
 *   j     0: (+29, +3, +7)   1: (-5, +31, -2)   2: (+11, -13, +37)   3: (-41, -17, +19)   4: (+23, -53, -43)   5: (-47, -59, -67)
 *         6: (+73, +61, -71)
 * INSIDE, for a point p and an odd K in {1, 3, 5, 7}: votes = the number of j < K for which the ray [p, DIRECTIONS[j], 0, +inf]
 * has an odd number of CROSSINGS; inside = 2 * votes > K.  A point with a non-finite coordinate: votes = 255, inside = 0.
 * A point outside a grid's box needs no special case: the space outside the box is empty.  A point ON the surface gets the side
 * the roundings give; an open mesh has no inside, and its votes tell how far the directions disagree; a ray through a shared
 * edge may count 0 or 2 there (no watertight edge rule), which the majority over K directions absorbs.
 *
 * nfl_mesh_crossings   one launch, a thread per ray of d_rays (n_rays, 8): d_count (n_rays) int32.  Brute and grid mode, the box
 *   and the mesh and grid arguments exactly as nfl_mesh_cast takes them.
 * nfl_mesh_inside      one launch, a thread per point of d_points (n, 3), the directions one after the other: d_votes (n) and,
 *   where given, d_inside (n), a byte each (uint8).  Brute and grid mode and their arguments as nfl_mesh_cast.
 *
 *   NFL_EINVAL (nothing launched): what nfl_mesh_cast refuses of n_rays / n, the mesh and the grid arguments; n_directions
 *   outside {1, 3, 5, 7}; for n > 0 a NULL or misaligned (4 B) d_rays, d_count or d_points, a NULL d_votes.  n == 0: NFL_OK, no
 *   launch. */
#define NFL_SOLID_MAX_DIRECTIONS 7
#define NFL_SOLID_DIRECTIONS {{5.38516474f, 1.73205078f, 2.64575124f}, {-2.23606801f, 5.56776428f, -1.41421354f}, \
                              {3.31662488f, -3.60555124f, 6.08276272f}, {-6.40312433f, -4.12310553f, 4.35889912f}, \
                              {4.79583168f, -7.28010988f, -6.55743837f}, {-6.85565472f, -7.68114567f, -8.18535233f}, \
                              {8.54400349f, 7.81024981f, -8.42614937f}}
int nfl_mesh_crossings(const float* d_rays, int64_t n_rays, const float* d_vertices, const int32_t* d_triangles,
                       int64_t n_vertices, int64_t n_triangles, const int64_t* d_offsets, const int32_t* d_entries,
                       int64_t n_entries, float lo_x, float lo_y, float lo_z, float cell, int32_t nx, int32_t ny, int32_t nz,
                       int32_t* d_count, void* stream);
int nfl_mesh_inside(const float* d_points, int64_t n, const float* d_vertices, const int32_t* d_triangles, int64_t n_vertices,
                    int64_t n_triangles, const int64_t* d_offsets, const int32_t* d_entries, int64_t n_entries,
                    float lo_x, float lo_y, float lo_z, float cell, int32_t nx, int32_t ny, int32_t nz, int32_t n_directions,
                    void* d_votes, void* d_inside, void* stream);

/* ---- mesh edges: the edge table of an indexed mesh, its boundary loops, and the caps that close them ------------------------
 * "mesh solid" is defined for a closed, consistently wound mesh.  This section tells whether a mesh is one, where it is open,
 * and closes it.  The mesh has V vertices and T triangles.  A triangle with an index outside [0, V) is counted and takes part
 * in nothing.
 *
 * HALF-EDGE h = 3 t + c, c in 0..2, runs from tri[t][c] to tri[t][(c + 1) % 3].  One whose two ends are equal is DEGENERATE: it
 * lies on no edge, has edge id -1 and is counted in n_degenerate.
 * EDGE: an unordered pair {a, b}, a < b, that has at least one half-edge.  Edges are numbered in ascending (a, b); E is their
 * number.  edges (E, 2) int32; half_edge (3T) int32, the edge of every half-edge or -1; edge_offsets (E + 1) int64 and
 * edge_halves (H) int32, the half-edges on each edge ASCENDING.  H = 3 T - n_degenerate for a mesh in range.
 * KIND (E) uint8: NFL_EDGE_INTERIOR exactly two half-edges, one in each direction; NFL_EDGE_BOUNDARY exactly one;
 * NFL_EDGE_FLIPPED exactly two in the same direction; NFL_EDGE_NONMANIFOLD three or more.
 * TWIN (3T) int32: the other half-edge of an INTERIOR edge, -1 everywhere else.
 * TOTALS of the edges, NFL_EDGE_TOTALS int64: E, H, n_boundary, n_flipped, n_nonmanifold (edges of each kind), n_degenerate,
 * and the number of triangles out of range.
 *
 * SUCCESSOR of a boundary half-edge h = (a -> b) of triangle t (one on a BOUNDARY edge).  Let g be the half-edge after h in t;
 * it starts at b.  While twin[g] >= 0: g becomes the half-edge after twin[g] in its triangle, which again starts at b.  If the
 * walk stops at a half-edge on a BOUNDARY edge, that is succ[h]; if it stops on a FLIPPED or NONMANIFOLD edge or at a
 * degenerate half-edge, or runs longer than 3 T steps (tables that are not this mesh's), succ[h] = -1.  The walk has an inverse,
 * so succ is a partial injection and the boundary half-edges fall into cycles and open chains.
 * LOOP: a cycle of succ.  Loops are numbered in ascending order of their smallest half-edge and listed from that half-edge
 * along succ.  loop_offsets (L + 1) int64, loop_halves (B') int32, loop_of (3T) int32 with -1 for a half-edge on no loop.  The
 * boundary half-edges on open chains are counted in n_open and belong to no loop.  A loop has at least 3 half-edges.
 * THE TABLE per loop: length int32; perimeter fp32 = the fp64 sum, in walk order, of the fp64 lengths sqrt((dx dx + dy dy) +
 * dz dz) of d = p_b - p_a taken in fp64 on the fp32 positions, rounded once; centroid (L, 3) fp32 = the fp64 sum, in walk
 * order, of the start vertices, divided by the length, rounded once.  A loop with a non-finite start vertex has perimeter =
 * +inf and centroid = 0 and is never filled.
 * TOTALS of the loops, NFL_LOOP_TOTALS int64: L, B', n_open.
 *
 * FILL.  A loop is SELECTED when its length is at least 3 and at most max_edges, its perimeter is finite and <= max_perimeter
 * (compared in fp32; +inf: no limit), and the byte of d_keep (L), where given, is not zero.  A selected loop of length 3
 * with half-edges a->b, b->c, c->a gets the ONE triangle (b, a, c) and no vertex.  A selected loop of length > 3 gets one new
 * vertex z and one triangle (b, a, z) per half-edge a -> b, in walk order.  z lies at the loop's centroid (the table's fp32,
 * bit for bit); its normal is the normalised fp64 sum, in walk order, of the new triangles' (p1 - p0) x (p2 - p0), zeros when
 * that sum is zero or not finite; its colour is the fp64 sum, in walk order, of the colours of the loop's start vertices over
 * the length, rounded once.  New vertices follow the V inputs in loop order; new triangles follow the T inputs in loop order and
 * then walk order; input rows are copied bit for bit.  Every new triangle runs against the boundary half-edge it covers, so
 * that edge becomes INTERIOR and the spokes of a fan are INTERIOR among themselves.
 * TOTALS of the fill, NFL_FILL_TOTALS int64: n_filled, n_new_vertices, n_new_triangles.
 *
 * nfl_mesh_edges_count   takes the vertex adjacency of "mesh smoothing" (d_offsets (V + 1), d_neighbors (n_neighbors): the
 *   sorted distinct neighbour rows).  Vertex a owns the edges to its neighbours b > a; a scan of those counts numbers the edges;
 *   a half-edge finds its edge by a binary search for max(a, b) in the row of min(a, b); a count per edge, a scan, a fill and a
 *   sort of each row (by its thread up to NFL_EDGE_SHORT_ROW half-edges, by the wave of its thread beyond) make the rows.
 *   Writes d_totals and the scratch (nfl_mesh_edges_bytes) that nfl_mesh_edges_emit reads, with E and H given back.
 * nfl_mesh_loops_count   takes the tables of the edges and n_boundary.  succ by a thread per half-edge; ceil(log2 n_boundary) + 1
 *   rounds of pointer doubling carry the smallest half-edge ahead and a dead end; a thread per loop walks it for the places and
 *   the sums.  Scratch: nfl_mesh_loops_bytes.  nfl_mesh_loops_emit takes L and B' given back.
 * nfl_mesh_fill_count    takes the loops' table and the selection; nfl_mesh_fill_emit the mesh, the loops and the totals, and
 *   writes the whole new mesh and, where given, a byte per output vertex and triangle: 1 = new.  d_colors and d_out_colors are
 *   both given or both NULL.  Scratch: nfl_mesh_fill_bytes(n_loops).
 * Everything read from the scratch or from a caller's table is bounded before it is used: tables that are not this mesh's
 * give wrong output, never an access out of range.
 *
 *   NFL_EINVAL (nothing launched): sizes negative or beyond int32 indices (n_vertices > INT32_MAX, n_triangles > INT32_MAX / 3,
 *   n_loops > INT32_MAX / 3), n_neighbors outside [0, 6 T]; a misaligned pointer (4 B, 8 B for int64); for a mesh that is not
 *   empty a NULL pointer that the sizes need; totals outside what the count can give (E, H, n_boundary, B' in [0, 3 T]; L in
 *   [0, T]; n_new_vertices in [0, L], n_new_triangles in [0, B']); max_edges < 3; max_perimeter not > 0.  NFL_ESMALL: a scratch
 *   below the _bytes size.  An empty mesh (V == 0 or T == 0; for the fill also L == 0): NFL_OK, no launch. */
#define NFL_EDGE_INTERIOR 0
#define NFL_EDGE_BOUNDARY 1
#define NFL_EDGE_FLIPPED 2
#define NFL_EDGE_NONMANIFOLD 3
#define NFL_EDGE_SHORT_ROW 8
#define NFL_EDGE_TOTALS 7
#define NFL_LOOP_TOTALS 3
#define NFL_FILL_TOTALS 3
size_t nfl_mesh_edges_bytes(int64_t n_vertices, int64_t n_triangles);
int nfl_mesh_edges_count(const int32_t* d_triangles, int64_t n_vertices, int64_t n_triangles, const int64_t* d_offsets,
                         const int32_t* d_neighbors, int64_t n_neighbors, void* d_scratch, size_t scratch_bytes,
                         int64_t* d_totals, void* stream);
int nfl_mesh_edges_emit(const int32_t* d_triangles, int64_t n_vertices, int64_t n_triangles, const void* d_scratch,
                        size_t scratch_bytes, int64_t n_edges, int64_t n_halves, int32_t* d_edges, int32_t* d_half_edge,
                        int64_t* d_edge_offsets, int32_t* d_edge_halves, void* d_kind, int32_t* d_twin, void* stream);
size_t nfl_mesh_loops_bytes(int64_t n_triangles);
int nfl_mesh_loops_count(const float* d_vertices, const int32_t* d_triangles, int64_t n_vertices, int64_t n_triangles,
                         const int32_t* d_half_edge, const int32_t* d_twin, const void* d_kind, int64_t n_edges,
                         int64_t n_boundary, void* d_scratch, size_t scratch_bytes, int64_t* d_totals, void* stream);
int nfl_mesh_loops_emit(int64_t n_triangles, const void* d_scratch, size_t scratch_bytes, int64_t n_loops,
                        int64_t n_loop_halves, int64_t* d_loop_offsets, int32_t* d_loop_halves, int32_t* d_loop_of,
                        int32_t* d_length, float* d_perimeter, float* d_centroid, void* stream);
size_t nfl_mesh_fill_bytes(int64_t n_loops);
int nfl_mesh_fill_count(int64_t n_loops, const int32_t* d_length, const float* d_perimeter, const void* d_keep,
                        int64_t max_edges, float max_perimeter, void* d_scratch, size_t scratch_bytes, int64_t* d_totals,
                        void* stream);
int nfl_mesh_fill_emit(const float* d_vertices, const float* d_normals, const float* d_colors, const int32_t* d_triangles,
                       int64_t n_vertices, int64_t n_triangles, const int64_t* d_loop_offsets, const int32_t* d_loop_halves,
                       const int32_t* d_loop_of, const float* d_centroid, int64_t n_loops, int64_t n_loop_halves,
                       const void* d_scratch, size_t scratch_bytes, int64_t n_new_vertices, int64_t n_new_triangles,
                       float* d_out_vertices, float* d_out_normals, float* d_out_colors, int32_t* d_out_triangles,
                       void* d_new_vertices, void* d_new_triangles, void* stream);

/* ---- hierarchical sampling (reference sample_pdf, rendering.py:7-46, plus the
 * concat + sort of rendering.py:267-272) -------------------------------------
 * d_z_coarse (R,S), d_weights_coarse (R,S); d_u (R,I) or NULL with d_u_row (I)
 * = linspace(0,1,I) shared by all rays (det).  Outputs: d_z_fine (R,S+I) sorted
 * ascending; d_samples (R,I) unsorted draws or NULL. */
int nfl_sample_pdf(const float* d_z_coarse, const float* d_weights_coarse,
                   const float* d_u, const float* d_u_row,
                   int32_t n_rays, int32_t n_samples, int32_t n_importance,
                   float* d_z_fine, float* d_samples, void* stream);

/* ---- misc ---------------------------------------------------------------- */
int         nfl_abi_version(void);
const char* nfl_version(void);        /* "nerf_fl_amd <x.y> gfx950 ..." */
const char* nfl_strerror(int code);
/* name of the dominant kernel of nfl_render_pass for (prec, n_emb_xyz), as it
 * appears in rocprofv3 kernel traces (used by bench.py to pair profiles) */
const char* nfl_render_kernel_name(int prec, int n_emb_xyz);

#ifdef __cplusplus
}
#endif
#endif /* NERF_FL_AMD_H */
