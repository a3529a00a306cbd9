// nfl_loss.hip -- NerfWLoss (reference losses.py:35-50) in two launches instead of ~8 + ~8 small ATen kernels:
//   c_l = coef 0.5 mean((rgb_coarse - t)^2)
//   f_l = coef 0.5 mean((rgb_fine - t)^2)                      without beta
//       = coef mean((rgb_fine - t)^2 / (2 beta^2)),  b_l = coef (3 + mean(log beta)),
//   s_l = coef lambda_u mean(transient_sigmas)                   with beta (NeRF-W)
// forward: the four terms, block-reduced and accumulated with one atomic per block and term;
// backward: the gradients of (go_c c_l + go_f f_l + go_b b_l + go_s s_l) w.r.t. the renderer's outputs, the go_k read
// from device scalars (what autograd hands over; a term nobody used has none and counts as 0).
#include <math.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_dev.h"

NFL_DEV float nfl_block_sum(float v, float* red) {
    v = nfl_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void nfl_loss_fwd_kernel(const nfl_loss_args a) {
    __shared__ float red[4];
    const long long n3 = (long long)a.n_rays * 3, nts = a.d_transient_sigmas ? (long long)a.n_rays * a.n_samples : 0;
    float c = 0.f, f = 0.f, b = 0.f, s = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (long long)gridDim.x * 256) {
        const float t = a.d_target[i];
        const float dc = a.d_rgb_coarse[i] - t;
        c += dc * dc;
        if (a.d_rgb_fine) {
            const float df = a.d_rgb_fine[i] - t;
            if (a.d_beta) {
                const float be = a.d_beta[i / 3];
                f += df * df / (2.f * be * be);
            } else {
                f += df * df;
            }
        }
    }
    if (a.d_beta)
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n_rays; i += (long long)gridDim.x * 256) b += logf(a.d_beta[i]);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nts; i += (long long)gridDim.x * 256) s += a.d_transient_sigmas[i];
    c = nfl_block_sum(c, red);
    f = nfl_block_sum(f, red);
    b = nfl_block_sum(b, red);
    s = nfl_block_sum(s, red);
    if (threadIdx.x == 0) {
        const float inv3 = 1.f / (float)n3;
        atomicAdd(a.d_losses + 0, a.coef * 0.5f * c * inv3);
        if (a.d_rgb_fine) atomicAdd(a.d_losses + 1, a.coef * (a.d_beta ? 1.f : 0.5f) * f * inv3);
        if (a.d_beta) {
            atomicAdd(a.d_losses + 2, a.coef * (b / (float)a.n_rays + (blockIdx.x == 0 ? 3.f : 0.f)));
            if (nts) atomicAdd(a.d_losses + 3, a.coef * a.lambda_u * s / (float)nts);
        }
    }
}

__global__ __launch_bounds__(256) void nfl_loss_bwd_kernel(const nfl_loss_args a) {
    const float go_c = a.d_grad_loss[0] ? *a.d_grad_loss[0] : 0.f, go_f = a.d_grad_loss[1] ? *a.d_grad_loss[1] : 0.f;
    const float go_b = a.d_grad_loss[2] ? *a.d_grad_loss[2] : 0.f, go_s = a.d_grad_loss[3] ? *a.d_grad_loss[3] : 0.f;
    const long long n3 = (long long)a.n_rays * 3, nts = a.d_g_transient_sigmas ? (long long)a.n_rays * a.n_samples : 0;
    const float inv3 = 1.f / (float)n3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (long long)gridDim.x * 256) {
        const float t = a.d_target[i];
        a.d_g_rgb_coarse[i] = go_c * a.coef * (a.d_rgb_coarse[i] - t) * inv3;
        if (a.d_rgb_fine) {
            const float df = a.d_rgb_fine[i] - t;
            if (a.d_beta) {
                const float be = a.d_beta[i / 3];
                a.d_g_rgb_fine[i] = go_f * a.coef * df / (be * be) * inv3;
            } else {
                a.d_g_rgb_fine[i] = go_f * a.coef * df * inv3;
            }
        }
    }
    if (a.d_beta)
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n_rays; i += (long long)gridDim.x * 256) {
            const float be = a.d_beta[i];
            float ss = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float df = a.d_rgb_fine[3 * i + k] - a.d_target[3 * i + k];
                ss += df * df;
            }
            a.d_g_beta[i] = a.coef * (-go_f * ss / (be * be * be) * inv3 + go_b / (be * (float)a.n_rays));
        }
    const float gs = nts ? go_s * a.coef * a.lambda_u / (float)nts : 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nts; i += (long long)gridDim.x * 256) a.d_g_transient_sigmas[i] = gs;
}

static int loss_args_ok(const nfl_loss_args* a) {
    if (!a || a->n_rays < 1 || !a->d_rgb_coarse || !a->d_target) return 0;
    if (a->d_beta && (!a->d_rgb_fine)) return 0;
    if (a->d_transient_sigmas && a->n_samples < 1) return 0;
    return 1;
}

__global__ void nfl_loss_zero_kernel(float* p) { if (threadIdx.x < 4) p[threadIdx.x] = 0.f; }

extern "C" int nfl_loss_forward(const nfl_loss_args* a, void* stream) {
    if (!loss_args_ok(a) || !a->d_losses) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // zeroed by a kernel, not hipMemsetAsync: a memset NODE of a captured graph was seen to take effect out of order with the
    // kernel after it when a second process replays graphs on the same GPU (nfl_compbwd.hip)
    hipLaunchKernelGGL(nfl_loss_zero_kernel, dim3(1), dim3(64), 0, s, a->d_losses);
    hipLaunchKernelGGL(nfl_loss_fwd_kernel, dim3(64), dim3(256), 0, s, *a);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}

extern "C" int nfl_loss_backward(const nfl_loss_args* a, void* stream) {
    if (!loss_args_ok(a) || !a->d_g_rgb_coarse || (a->d_rgb_fine && !a->d_g_rgb_fine) || (a->d_beta && !a->d_g_beta)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_loss_bwd_kernel, dim3(256), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
