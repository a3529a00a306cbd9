// nfl_appearance.hip -- fitting NeRF-W appearance codes to images the fields were not trained on (the paper's
// Phototourism protocol: optimise the code of a test image on some of its pixels).  include/nerf_fl_amd.h,
// "appearance codes of unseen images", has the algebra; DESIGN.md section 14 the measurements.
//
//   nfl_appearance_cache   one fine render pass (NFL_MODE_ZCACHE of the fused render kernel) that also writes the
//                          pre-activation Z of dir_encoding.0 with a zero appearance input: everything but the colour
//                          branch is then constant across fit iterations
//   nfl_appearance_fit     one iteration: fit kernel (stream Z, forward + backward of the colour branch, per-item
//                          partials) + reduce kernel (per-image sums in a fixed order, W_a^T, loss).  No atomics.
//
// Cache layout [ray][feature][sample], sample stride n_pad (a multiple of 64): lane l of a wavefront owns sample
// 64 ch + l of the ray, so every feature row is one coalesced 256 B read per wavefront.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_dev.h"
#include "nfl_launch.h"      // the cache entry's checks, NFL_AF_MAXCH

extern "C" int nfl_launch_zcache_x3(const NflPlan*, const void*, const void*, const nfl_pass_args*, float*, int, void*);

#define NFL_AF_F 128          // output width of dir_encoding.0

typedef float nfl_af4 __attribute__((ext_vector_type(4)));

// One wavefront per work item (a ray range of one image).  Per ray: all chunks of 64 samples forward (the relu masks,
// the sample colours and w_s stay in registers), the composited colour and its MSE gradient, then the backward of the
// chunks into 128 per-lane accumulators that live across all the item's rays.
template <int NCH>
__global__ __launch_bounds__(256) void nfl_appfit_kernel(const nfl_appfit_args A, float gscale) {
    constexpr int NP = 64 * NCH;
    __shared__ nfl_af4 tab[4][NFL_AF_F];        // per wavefront: {u_f, W_rgb[0][f], W_rgb[1][f], W_rgb[2][f]}
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    const bool live = item < A.n_items;
    const int it = live ? item : A.n_items - 1;
    const int img = A.d_items[3 * it], r0 = A.d_items[3 * it + 1], r1 = live ? A.d_items[3 * it + 2] : r0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {              // u_i = W_a a_i: two features per lane
        const int f = lane + 64 * q;
        const float* w = A.d_w_dir + (size_t)f * A.ld_dir + A.col_a;
        const float* a = A.d_codes + (size_t)img * A.n_a;
        float u = 0.f;
        for (int k = 0; k < A.n_a; ++k) u = fmaf(w[k], a[k], u);
        tab[wave][f] = nfl_af4{u, A.d_w_rgb[f], A.d_w_rgb[NFL_AF_F + f], A.d_w_rgb[2 * NFL_AF_F + f]};
    }
    __syncthreads();
    const float b0 = A.d_b_rgb[0], b1 = A.d_b_rgb[1], b2 = A.d_b_rgb[2];
    const int N = A.n_samples;
    float acc[NFL_AF_F];
#pragma unroll
    for (int f = 0; f < NFL_AF_F; ++f) acc[f] = 0.f;
    float sq = 0.f;
    // features per scheduling block: bounds the loads the compiler keeps in flight (FB * NCH registers) beside the
    // 128 accumulators
    constexpr int FB = NCH <= 2 ? 16 : 8;
    for (int r = r0; r < r1; ++r) {
        unsigned msk[NCH][4];
        float rgb[NCH][3], ws[NCH];
        bool ok[NCH];
        const float* zp = A.d_zcache + (size_t)r * NFL_AF_F * NP + lane;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            ok[ch] = 64 * ch + lane < N;
            ws[ch] = ok[ch] ? A.d_weights[(size_t)r * N + 64 * ch + lane] : 0.f;
            rgb[ch][0] = b0;
            rgb[ch][1] = b1;
            rgb[ch][2] = b2;
#pragma unroll
            for (int q = 0; q < 4; ++q) msk[ch][q] = 0u;
        }
#pragma unroll
        for (int f0 = 0; f0 < NFL_AF_F; f0 += FB) {
#pragma unroll
            for (int f = f0; f < f0 + FB; ++f) {
                const nfl_af4 t = tab[wave][f];
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    // the padding samples are never written: not read
                    const float z = ok[ch] ? zp[(size_t)f * NP + 64 * ch] : 0.f;
                    const float p = z + t[0];
                    const bool on = p > 0.f;
                    const float hh = on ? p : 0.f;
                    msk[ch][f >> 5] |= (unsigned)on << (f & 31);
                    rgb[ch][0] = fmaf(t[1], hh, rgb[ch][0]);
                    rgb[ch][1] = fmaf(t[2], hh, rgb[ch][1]);
                    rgb[ch][2] = fmaf(t[3], hh, rgb[ch][2]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int k = 0; k < 3; ++k) rgb[ch][k] = 1.f / (1.f + expf(-rgb[ch][k]));
            c0 = fmaf(ws[ch], rgb[ch][0], c0);
            c1 = fmaf(ws[ch], rgb[ch][1], c1);
            c2 = fmaf(ws[ch], rgb[ch][2], c2);
        }
        c0 = nfl_wave_sum(c0);
        c1 = nfl_wave_sum(c1);
        c2 = nfl_wave_sum(c2);
        if (A.white_back) {
            const float wb = 1.f - A.d_opacity[r];
            c0 += wb;
            c1 += wb;
            c2 += wb;
        }
        if (A.d_rgb && lane < 3) A.d_rgb[(size_t)r * 3 + lane] = lane == 0 ? c0 : (lane == 1 ? c1 : c2);
        const float* tg = A.d_target + (size_t)r * 3;
        const float d0 = c0 - tg[0], d1 = c1 - tg[1], d2 = c2 - tg[2];
        sq += d0 * d0 + d1 * d1 + d2 * d2;
        const float g0 = gscale * d0, g1 = gscale * d1, g2 = gscale * d2;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {      // rgb <- w_s g_r . rgb_s . (1 - rgb_s)
            rgb[ch][0] = ws[ch] * g0 * (rgb[ch][0] * (1.f - rgb[ch][0]));
            rgb[ch][1] = ws[ch] * g1 * (rgb[ch][1] * (1.f - rgb[ch][1]));
            rgb[ch][2] = ws[ch] * g2 * (rgb[ch][2] * (1.f - rgb[ch][2]));
        }
#pragma unroll
        for (int f0 = 0; f0 < NFL_AF_F; f0 += 16) {
#pragma unroll
            for (int f = f0; f < f0 + 16; ++f) {
                const nfl_af4 t = tab[wave][f];
                float d = 0.f;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const float e = fmaf(t[1], rgb[ch][0], fmaf(t[2], rgb[ch][1], t[3] * rgb[ch][2]));
                    d += ((msk[ch][f >> 5] >> (f & 31)) & 1u) ? e : 0.f;
                }
                acc[f] += d;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the item's sum over its samples: lane l keeps features l and 64 + l, then two coalesced stores
    float lo = 0.f, hi = 0.f;
#pragma unroll
    for (int f = 0; f < NFL_AF_F; ++f) {
        const float t = nfl_wave_sum(acc[f]);
        if (f < 64) lo = lane == f ? t : lo;
        else hi = lane == f - 64 ? t : hi;
    }
    if (live) {
        A.d_partials[(size_t)it * NFL_AF_F + lane] = lo;
        A.d_partials[(size_t)it * NFL_AF_F + 64 + lane] = hi;
        if (lane == 0) A.d_partials[(size_t)A.n_items * NFL_AF_F + it] = sq;
    }
}

// blocks 0 .. n_images-1: one image each (its items in order, then W_a^T); block n_images: the loss
__global__ __launch_bounds__(NFL_AF_F) void nfl_appfit_reduce_kernel(const nfl_appfit_args A, float inv3r) {
    __shared__ float s[NFL_AF_F];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b < A.n_images) {
        const int i0 = A.d_image_items[b], i1 = A.d_image_items[b + 1];
        float v = 0.f;
        for (int it = i0; it < i1; ++it) v += A.d_partials[(size_t)it * NFL_AF_F + t];
        s[t] = v;
        __syncthreads();
        if (t < A.n_a) {
            float g = 0.f;
            for (int f = 0; f < NFL_AF_F; ++f) g = fmaf(A.d_w_dir[(size_t)f * A.ld_dir + A.col_a + t], s[f], g);
            A.d_grad[(size_t)b * A.n_a + t] = g;
        }
    } else {
        float v = 0.f;
        for (int it = t; it < A.n_items; it += NFL_AF_F) v += A.d_partials[(size_t)A.n_items * NFL_AF_F + it];
        s[t] = v;
        __syncthreads();
        for (int w = NFL_AF_F / 2; w >= 1; w >>= 1) {
            if (t < w) s[t] += s[t + w];
            __syncthreads();
        }
        if (t == 0) A.d_loss[0] = s[0] * inv3r;
    }
}

template <int NCH>
static void nfl_launch_appfit(const nfl_appfit_args& A, float gscale, hipStream_t s) {
    hipLaunchKernelGGL(nfl_appfit_kernel<NCH>, dim3((A.n_items + 3) / 4), dim3(256), 0, s, A, gscale);
}

extern "C" {

int nfl_appearance_cache(const void* h_plan, const void* d_plan, const void* d_packed, const nfl_pass_args* a,
                         float* d_zcache, int32_t n_pad, void* stream) {
    const NflPlan* hp = static_cast<const NflPlan*>(h_plan);
    int launch = 0;
    const int rc = nfl_render_check(NFL_ENTRY_CACHE, hp, d_plan, d_packed, a, d_zcache, n_pad, &launch);
    if (!launch) return rc;
    return nfl_launch_zcache_x3(hp, d_plan, d_packed, a, d_zcache, n_pad, stream);
}

size_t nfl_appfit_partials_floats(int32_t n_items) { return n_items < 0 ? 0 : (size_t)n_items * (NFL_AF_F + 1); }

int nfl_appearance_fit(const nfl_appfit_args* A, void* stream) {
    if (!A) return NFL_EINVAL;
    if (A->n_rays < 0 || A->n_items < 0 || A->n_images < 0 || A->n_samples < 1) return NFL_EINVAL;
    if (A->n_pad < A->n_samples || A->n_pad % 64 != 0 || A->n_pad > 64 * NFL_AF_MAXCH) return NFL_EINVAL;
    if (A->n_a < 1 || A->n_a > NFL_AF_F || A->col_a < 0 || A->ld_dir < A->col_a + A->n_a) return NFL_EINVAL;
    if (!A->d_codes || !A->d_w_dir || !A->d_grad || !A->d_loss || !A->d_image_items) return NFL_EINVAL;
    if (A->n_items > 0 && (!A->d_zcache || !A->d_weights || !A->d_target || !A->d_items || !A->d_partials ||
                           !A->d_w_rgb || !A->d_b_rgb || (A->white_back && !A->d_opacity)))
        return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float gscale = A->n_rays > 0 ? 2.f / (3.f * (float)A->n_rays) : 0.f;
    const float inv3r = A->n_rays > 0 ? 1.f / (3.f * (float)A->n_rays) : 0.f;
    if (A->n_items > 0) {
        switch (A->n_pad / 64) {
            case 1: nfl_launch_appfit<1>(*A, gscale, s); break;
            case 2: nfl_launch_appfit<2>(*A, gscale, s); break;
            case 3: nfl_launch_appfit<3>(*A, gscale, s); break;
            default: nfl_launch_appfit<4>(*A, gscale, s); break;
        }
        if (hipGetLastError() != hipSuccess) return NFL_ELAUNCH;
    }
    hipLaunchKernelGGL(nfl_appfit_reduce_kernel, dim3(A->n_images + 1), dim3(NFL_AF_F), 0, s, *A, inv3r);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}

}  // extern "C"
