// nfl_optim.hip -- optimiser steps over a list of parameter tensors in one launch: Adam (nfl_adam_step), and SGD, Adam with
// weight decay, RAdam and Ranger (nfl_optim_step, further down).
//
// The reference optimises with torch.optim.Adam(lr, eps=1e-8) (utils/__init__.py:30-32); under PyTorch that is
// ~7 multi-tensor kernels per step (110 us next to a 5.7 ms train step); its single-kernel `fused=True` variant
// does not move the parameters' version counters, which render_rays keys its weight re-pack on
// (nerf_fl_amd/train.py).  Same arithmetic
// as torch's default implementation, in its order:
//   m += (g - m) (1 - b1);  v = v b2 + (1 - b2) g g;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound: 16 B read + 12 B written per parameter.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/nerf_fl_amd.h"

__global__ __launch_bounds__(256) void nfl_adam_kernel(const nfl_adam_tensors T, const float one_minus_b1, const float b2,
                                                       const float one_minus_b2, const float step_size,
                                                       const float bc2_sqrt, const float eps) {
    const int t = blockIdx.y;
    const float* g = T.grad[t];
    if (g == nullptr) return;                    // parameter without a gradient this step: untouched, as in torch
    float* p = T.param[t];
    float* m = T.exp_avg[t];
    float* v = T.exp_avg_sq[t];
    const int n = T.numel[t];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float gi = g[i];
        const float mi = m[i] + (gi - m[i]) * one_minus_b1;
        const float vi = v[i] * b2 + one_minus_b2 * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
}

extern "C" int nfl_adam_step(const nfl_adam_tensors* t, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                             int32_t step, void* stream) {
    if (!t || n_tensors < 0 || n_tensors > NFL_ADAM_MAX_TENSORS || step < 1) return NFL_EINVAL;
    if (n_tensors == 0) return NFL_OK;
    for (int i = 0; i < n_tensors; ++i)
        if (t->numel[i] < 0 || (t->numel[i] > 0 && (!t->param[i] || !t->exp_avg[i] || !t->exp_avg_sq[i]))) return NFL_EINVAL;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(nfl_adam_kernel, dim3(32, n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream), *t,
                       1.0f - beta1, beta2, 1.0f - beta2, (float)((double)lr / bc1), (float)sqrt(bc2), eps);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}

// Graph-capturable form: learning rate, betas, eps and the step count are read from device memory by the kernel, so
// one captured launch stays valid while a scheduler changes the rate and the count advances with every replay.
__global__ __launch_bounds__(256) void nfl_adam_dev_kernel(const nfl_adam_tensors T, const float* __restrict__ hyper,
                                                           const int32_t* __restrict__ d_step) {
    const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3];
    const int step = *d_step + 1;
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
    const float one_minus_b1 = 1.0f - b1, one_minus_b2 = 1.0f - b2;
    const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const int t = blockIdx.y;
    const float* g = T.grad[t];
    if (g == nullptr) return;
    float* p = T.param[t];
    float* m = T.exp_avg[t];
    float* v = T.exp_avg_sq[t];
    const int n = T.numel[t];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float gi = g[i];
        const float mi = m[i] + (gi - m[i]) * one_minus_b1;
        const float vi = v[i] * b2 + one_minus_b2 * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
}
__global__ void nfl_adam_bump_kernel(int32_t* d_step) { *d_step += 1; }

extern "C" int nfl_adam_step_dev(const nfl_adam_tensors* t, int32_t n_tensors, const float* d_hyper, int32_t* d_step,
                                 int32_t bump, void* stream) {
    if (!t || n_tensors < 0 || n_tensors > NFL_ADAM_MAX_TENSORS || !d_hyper || !d_step) return NFL_EINVAL;
    if (n_tensors == 0) return NFL_OK;
    for (int i = 0; i < n_tensors; ++i)
        if (t->numel[i] < 0 || (t->numel[i] > 0 && (!t->param[i] || !t->exp_avg[i] || !t->exp_avg_sq[i]))) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_adam_dev_kernel, dim3(32, n_tensors), dim3(256), 0, static_cast<hipStream_t>(stream), *t, d_hyper,
                       d_step);
    if (bump) hipLaunchKernelGGL(nfl_adam_bump_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), d_step);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------
// SGD (momentum, weight decay), Adam with weight decay, RAdam and Ranger over up to NFL_ADAM_MAX_TENSORS tensors in one
// launch (nfl_optim_step / nfl_optim_step_dev; include/nerf_fl_amd.h states the arithmetic of every kind).
// The kind is a template parameter: the element loop has no branch on it.  What depends on the step count (bias
// corrections, RAdam's N_sma and step size, Ranger's lookahead flag) is computed once per launch in fp64 from the fp32
// hyper-parameters by the same code in both forms (by every thread, while its first loads are in flight), so a captured
// launch and an eager one round identically.
// Elementwise, no atomics, no reduction: the result is a function of the inputs only, on every rank.
// HBM-bound: 16-byte loads and stores whenever all of a tensor's pointers are 16-byte aligned, a scalar tail after them.
struct nfl_opt_hyper {
    float h[NFL_OPT_HYPER];  // lr, beta1 | momentum, beta2, eps, weight_decay, alpha, k, threshold
    int32_t step;            // 1-based
};

struct nfl_opt_scalars {
    float a, b, c, d, e, f;  // per kind, see nfl_opt_prepare
    float wd;                // L2 coefficient (SGD, Adam) or the decoupled decay lr * wd (RAdam, Ranger)
    float alpha;             // Ranger: lookahead step
    int rect;                // RAdam / Ranger: rectified branch
    int sync;                // Ranger: lookahead synchronisation after this update
};

template <int KIND>
__device__ nfl_opt_scalars nfl_opt_prepare(const float* h, int step) {
    nfl_opt_scalars s = {};
    const float lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
    if (KIND == NFL_OPT_SGD) {
        s.a = lr;
        s.b = b1;  // momentum
        s.wd = wd;
    } else if (KIND == NFL_OPT_ADAM) {  // nfl_adam_kernel's scalars, rounded the same way
        const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
        s.a = 1.0f - b1;
        s.b = b2;
        s.c = 1.0f - b2;
        s.d = (float)((double)lr / bc1);
        s.e = (float)sqrt(bc2);
        s.f = eps;
        s.wd = wd;
    } else {  // RAdam, Ranger
        const double B2 = (double)b2, b2t = pow(B2, (double)step), bc1 = 1.0 - pow((double)b1, (double)step);
        const double n_max = 2.0 / (1.0 - B2) - 1.0, n = n_max - 2.0 * (double)step * b2t / (1.0 - b2t);
        const double thr = (double)h[7];
        s.rect = KIND == NFL_OPT_RADAM ? n >= thr : n > thr;
        const double r = s.rect ? sqrt((1.0 - b2t) * (n - 4.0) / (n_max - 4.0) * (n - 2.0) / n * n_max / (n_max - 2.0)) : 1.0;
        s.a = b1;
        s.b = 1.0f - b1;
        s.c = b2;
        s.d = 1.0f - b2;
        s.e = (float)((double)lr * r / bc1);
        s.f = eps;
        s.wd = (float)((double)wd * (double)lr);
        if (KIND == NFL_OPT_RANGER) {
            const int k = (int)h[6];
            s.alpha = h[5];
            s.sync = k >= 1 && step % k == 0;
        }
    }
    return s;
}

// one element: parameter p, gradient g, the kind's state m (exp_avg | momentum_buffer), v (exp_avg_sq), w (slow_buffer)
template <int KIND>
__device__ __forceinline__ void nfl_opt_elem(float& p, float g, float& m, float& v, float& w, const nfl_opt_scalars& s,
                                             bool momentum) {
    if (KIND == NFL_OPT_SGD) {
        if (s.wd != 0.f) g = g + s.wd * p;
        if (momentum) {  // the buffer starts at zero, so the first update makes it g exactly (torch: buf = clone(g))
            m = s.b * m + g;
            g = m;
        }
        p = p - s.a * g;
    } else if (KIND == NFL_OPT_ADAM) {  // nfl_adam_kernel's expressions
        if (s.wd != 0.f) g = g + s.wd * p;
        const float mi = m + (g - m) * s.a;
        const float vi = v * s.b + s.c * g * g;
        m = mi;
        v = vi;
        p = p - s.d * (mi / (sqrtf(vi) / s.e + s.f));
    } else {
        const float vi = s.c * v + s.d * g * g;
        const float mi = s.a * m + s.b * g;
        v = vi;
        m = mi;
        if (s.wd != 0.f) p = p - s.wd * p;
        p = s.rect ? p - s.e * (mi / (sqrtf(vi) + s.f)) : p - s.e * mi;
        if (KIND == NFL_OPT_RANGER && s.sync) {
            w = w + s.alpha * (p - w);
            p = w;
        }
    }
}

template <int KIND>
__device__ __forceinline__ void nfl_opt_elem4(float4& p, const float4 g, float4& m, float4& v, float4& w,
                                              const nfl_opt_scalars& s, bool momentum) {
    nfl_opt_elem<KIND>(p.x, g.x, m.x, v.x, w.x, s, momentum);
    nfl_opt_elem<KIND>(p.y, g.y, m.y, v.y, w.y, s, momentum);
    nfl_opt_elem<KIND>(p.z, g.z, m.z, v.z, w.z, s, momentum);
    nfl_opt_elem<KIND>(p.w, g.w, m.w, v.w, w.w, s, momentum);
}

// d_hyper == NULL: the by-value scalars `hv`; otherwise float[NFL_OPT_HYPER] at d_hyper and step *d_step + 1.
// Every thread issues its first loads before the fp64 scalars are computed, so their latency hides that arithmetic.
template <int KIND>
__global__ __launch_bounds__(256) void nfl_optim_kernel(const nfl_optim_tensors T, const nfl_opt_hyper hv,
                                                        const float* __restrict__ d_hyper,
                                                        const int32_t* __restrict__ d_step) {
    const int t = blockIdx.y;
    const float* __restrict__ g = T.grad[t];
    if (g == nullptr) return;  // parameter without a gradient this step: untouched, as in torch
    float* __restrict__ p = T.param[t];
    // SGD: state0 is the momentum buffer, NULL without momentum; the other kinds use what they need and ignore the rest
    float* __restrict__ m = T.state0[t];
    float* __restrict__ v = KIND == NFL_OPT_SGD ? nullptr : T.state1[t];
    float* __restrict__ w = KIND == NFL_OPT_RANGER ? T.state2[t] : nullptr;
    const bool momentum = KIND != NFL_OPT_SGD || m != nullptr;
    const int n = T.numel[t];
    const uintptr_t align = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)w;
    const int n4 = (align & 15) == 0 ? n >> 2 : 0;
    const int stride = gridDim.x * 256;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int i = blockIdx.x * 256 + threadIdx.x;
    float4 pi = z4, gi = z4, mi = z4, vi = z4, wi = z4;
    if (i < n4) {
        pi = reinterpret_cast<const float4*>(p)[i];
        gi = reinterpret_cast<const float4*>(g)[i];
        if (m) mi = reinterpret_cast<const float4*>(m)[i];
        if (v) vi = reinterpret_cast<const float4*>(v)[i];
    }
    float h[NFL_OPT_HYPER];
#pragma unroll
    for (int k = 0; k < NFL_OPT_HYPER; ++k) h[k] = d_hyper ? d_hyper[k] : hv.h[k];
    const nfl_opt_scalars s = nfl_opt_prepare<KIND>(h, d_hyper ? *d_step + 1 : hv.step);
    w = s.sync ? w : nullptr;  // the slow buffer is touched on synchronisation steps only
    while (i < n4) {
        if (w) wi = reinterpret_cast<const float4*>(w)[i];
        nfl_opt_elem4<KIND>(pi, gi, mi, vi, wi, s, momentum);
        reinterpret_cast<float4*>(p)[i] = pi;
        if (m) reinterpret_cast<float4*>(m)[i] = mi;
        if (v) reinterpret_cast<float4*>(v)[i] = vi;
        if (w) reinterpret_cast<float4*>(w)[i] = wi;
        i += stride;
        if (i < n4) {
            pi = reinterpret_cast<const float4*>(p)[i];
            gi = reinterpret_cast<const float4*>(g)[i];
            if (m) mi = reinterpret_cast<const float4*>(m)[i];
            if (v) vi = reinterpret_cast<const float4*>(v)[i];
        }
    }
    for (int j = 4 * n4 + blockIdx.x * 256 + threadIdx.x; j < n; j += stride) {
        float pj = p[j], mj = m ? m[j] : 0.f, vj = v ? v[j] : 0.f, wj = w ? w[j] : 0.f;
        nfl_opt_elem<KIND>(pj, g[j], mj, vj, wj, s, momentum);
        p[j] = pj;
        if (m) m[j] = mj;
        if (v) v[j] = vj;
        if (w) w[j] = wj;
    }
}

// host-side checks shared by both forms; `momentum` < 0: unknown (device-side hyper-parameters)
static int nfl_optim_args_ok(const nfl_optim_tensors* t, int32_t n, int32_t kind, float momentum) {
    if (!t || n < 0 || n > NFL_ADAM_MAX_TENSORS || kind < NFL_OPT_SGD || kind > NFL_OPT_RANGER) return 0;
    for (int i = 0; i < n; ++i) {
        if (t->numel[i] < 0) return 0;
        if (t->numel[i] == 0) continue;
        if (!t->param[i]) return 0;
        if (kind == NFL_OPT_SGD && momentum > 0.f && !t->state0[i]) return 0;
        if (kind != NFL_OPT_SGD && (!t->state0[i] || !t->state1[i])) return 0;
        if (kind == NFL_OPT_RANGER && !t->state2[i]) return 0;
    }
    return 1;
}

static void nfl_optim_launch(const nfl_optim_tensors* t, int32_t n, int32_t kind, const nfl_opt_hyper& hv,
                             const float* d_hyper, const int32_t* d_step, hipStream_t s) {
    const dim3 grid(32, n), block(256);
    switch (kind) {
        case NFL_OPT_SGD: hipLaunchKernelGGL(nfl_optim_kernel<NFL_OPT_SGD>, grid, block, 0, s, *t, hv, d_hyper, d_step); break;
        case NFL_OPT_ADAM: hipLaunchKernelGGL(nfl_optim_kernel<NFL_OPT_ADAM>, grid, block, 0, s, *t, hv, d_hyper, d_step); break;
        case NFL_OPT_RADAM: hipLaunchKernelGGL(nfl_optim_kernel<NFL_OPT_RADAM>, grid, block, 0, s, *t, hv, d_hyper, d_step); break;
        default: hipLaunchKernelGGL(nfl_optim_kernel<NFL_OPT_RANGER>, grid, block, 0, s, *t, hv, d_hyper, d_step); break;
    }
}

extern "C" int nfl_optim_step(const nfl_optim_tensors* t, int32_t n_tensors, int32_t kind, const float* hyper, int32_t step,
                              void* stream) {
    if (!hyper || step < 1 || !nfl_optim_args_ok(t, n_tensors, kind, kind == NFL_OPT_SGD ? hyper[1] : 0.f)) return NFL_EINVAL;
    if (kind == NFL_OPT_SGD && hyper[1] < 0.f) return NFL_EINVAL;
    if (kind == NFL_OPT_RANGER && !(hyper[6] >= 1.f)) return NFL_EINVAL;
    if (n_tensors == 0) return NFL_OK;
    nfl_opt_hyper hv;
    for (int k = 0; k < NFL_OPT_HYPER; ++k) hv.h[k] = hyper[k];
    hv.step = step;
    nfl_optim_launch(t, n_tensors, kind, hv, nullptr, nullptr, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}

extern "C" int nfl_optim_step_dev(const nfl_optim_tensors* t, int32_t n_tensors, int32_t kind, const float* d_hyper,
                                  int32_t* d_step, int32_t bump, void* stream) {
    if (!d_hyper || !d_step || !nfl_optim_args_ok(t, n_tensors, kind, 0.f)) return NFL_EINVAL;
    if (n_tensors == 0) return NFL_OK;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    nfl_optim_launch(t, n_tensors, kind, nfl_opt_hyper{}, d_hyper, d_step, s);
    if (bump) hipLaunchKernelGGL(nfl_adam_bump_kernel, dim3(1), dim3(1), 0, s, d_step);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
