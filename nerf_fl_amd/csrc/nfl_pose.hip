// nfl_pose.hip -- learnable camera poses for --refine_pose: per-camera (r, t) deltas -> world rays, and back.
//
// Forward (reference models/poses.py:27-34, utils/lie_group_helper.py:63-84, datasets/ray_utils.py:29-55): one thread per
// ray looks its camera up (image id -> pose row), evaluates Exp(r) as the reference writes it (n = |r| + 1e-15,
// sin(n)/n, (1 - cos n)/n^2; 3x3 algebra is ~60 flops, cheaper per ray than a second launch per camera), composes with
// init_c2w, rotates and normalises the camera-frame direction and writes the (8)-float row render_rays takes.
//
// Backward: one wavefront per camera.  Its 64 lanes scan the per-ray pose rows the forward wrote; lane l sums the
// rays l, l + 64, l + 128, ... of its camera in index order into dL/dc2w (12 floats), a fixed xor butterfly combines the
// lanes, and lane 0 chains through init_c2w and Rodrigues and WRITES dL/dr, dL/dt (0 for a camera no ray uses).  No
// atomics and no scratch: the order of every sum depends on the inputs only, so repeated calls are bit-identical, and a
// camera's gradient is complete when its wave ends.  The scan costs n_cams x n_rays int32 compares (1500 x 1024 from L2
// at the configs[3] shape); a bucketing sort would need a scan + scatter (two more launches and scratch) to save that.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_dev.h"

namespace {

// c2w[:3, :] of camera `c` as the reference builds it: make_c2w(r, t) @ init_c2w (row-major 3x4)
__device__ __forceinline__ void nfl_pose_c2w(const nfl_pose_args& a, int c, float P[12]) {
    const float r0 = a.d_r[3 * c], r1 = a.d_r[3 * c + 1], r2 = a.d_r[3 * c + 2];
    const float n = sqrtf(r0 * r0 + r1 * r1 + r2 * r2) + 1e-15f;
    const float al = sinf(n) / n, be = (1.f - cosf(n)) / (n * n);
    const float K[9] = {0.f, -r2, r1, r2, 0.f, -r0, -r1, r0, 0.f};
    float R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float kk = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
            R[3 * i + j] = ((i == j ? 1.f : 0.f) + al * K[3 * i + j]) + be * kk;
        }
    const float t[3] = {a.d_t[3 * c], a.d_t[3 * c + 1], a.d_t[3 * c + 2]};
    if (a.d_init_c2w) {
        const float* A = a.d_init_c2w + (size_t)16 * c;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                P[4 * i + j] = R[3 * i] * A[j] + R[3 * i + 1] * A[4 + j] + R[3 * i + 2] * A[8 + j] + t[i] * A[12 + j];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            P[4 * i] = R[3 * i];
            P[4 * i + 1] = R[3 * i + 1];
            P[4 * i + 2] = R[3 * i + 2];
            P[4 * i + 3] = t[i];
        }
    }
}

__global__ __launch_bounds__(256) void nfl_pose_rays_kernel(const nfl_pose_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rays) return;
    const long long id = a.d_ts[i];
    int c = -1;
    if (id >= 0 && id < a.n_ids) {
        const long long row = a.d_row_of_id[id];
        if (row >= 0 && row < a.n_cams) c = (int)row;
    }
    a.d_rows[i] = c;
    float* out = a.d_rays + (size_t)i * 8;
    if (c < 0) {
        const float q = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = q;
        if (a.d_status) atomicOr(a.d_status, NFL_STATUS_POSE_ID);
        return;
    }
    float P[12];
    nfl_pose_c2w(a, c, P);
    const float* rc = a.d_rays_cam + (size_t)i * a.cam_stride;
    const float x = rc[0], y = rc[1], z = rc[2];
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = x * P[4 * k] + y * P[4 * k + 1] + z * P[4 * k + 2];
    const float nv = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    out[0] = P[3];
    out[1] = P[7];
    out[2] = P[11];
    out[3] = v[0] / nv;
    out[4] = v[1] / nv;
    out[5] = v[2] / nv;
    out[6] = rc[3];
    out[7] = rc[4];
}

// sin(n)/n, (1 - cos n)/n^2 and their derivatives, without the cancellation of the closed forms below n = 0.1 (where the
// series' first omitted terms are < 1e-13); the closed forms beyond
__device__ __forceinline__ void nfl_rodrigues_coeffs(float n, float& al, float& be, float& dal, float& dbe) {
    if (n < 0.1f) {
        const float n2 = n * n;
        al = 1.f - n2 * (1.f / 6.f - n2 * (1.f / 120.f - n2 * (1.f / 5040.f)));
        be = 0.5f - n2 * (1.f / 24.f - n2 * (1.f / 720.f - n2 * (1.f / 40320.f)));
        dal = -n * (1.f / 3.f - n2 * (1.f / 30.f - n2 * (1.f / 840.f)));
        dbe = -n * (1.f / 12.f - n2 * (1.f / 180.f - n2 * (1.f / 6720.f)));
    } else {
        const float s = sinf(n), co = cosf(n);
        al = s / n;
        be = (1.f - co) / (n * n);
        dal = (n * co - s) / (n * n);
        dbe = s / (n * n) - 2.f * (1.f - co) / (n * n * n);
    }
}

__global__ __launch_bounds__(256) void nfl_pose_rays_bwd_kernel(const nfl_pose_args a) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.n_cams) return;                     // whole wavefronts: the shuffles below see all 64 lanes
    float P[12];
    nfl_pose_c2w(a, c, P);
    float G[12];                                   // dL/dP, same layout as P
#pragma unroll
    for (int k = 0; k < 12; ++k) G[k] = 0.f;
    for (int i = lane; i < a.n_rays; i += 64) {
        if (a.d_rows[i] != c) continue;
        const float* rc = a.d_rays_cam + (size_t)i * a.cam_stride;
        const float* g = a.d_g_rays + (size_t)i * 8;
        const float dir[3] = {rc[0], rc[1], rc[2]};
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = dir[0] * P[4 * k] + dir[1] * P[4 * k + 1] + dir[2] * P[4 * k + 2];
        const float nv = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const float d[3] = {v[0] / nv, v[1] / nv, v[2] / nv};
        const float dg = d[0] * g[3] + d[1] * g[4] + d[2] * g[5];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gv = (g[3 + k] - d[k] * dg) / nv;         // (I - d d^T) g_d / |v|
            G[4 * k] += gv * dir[0];
            G[4 * k + 1] += gv * dir[1];
            G[4 * k + 2] += gv * dir[2];
            G[4 * k + 3] += g[k];                                 // origin = c2w[:3, 3]
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) G[k] = nfl_wave_sum(G[k]);
    if (lane) return;

    // through c2w[:3] = [R | t] @ init_c2w:  dL/dR_ik = sum_j G_ij init[k, j];  dL/dt_i = sum_j G_ij init[3, j]
    float GR[9], gt[3];
    if (a.d_init_c2w) {
        const float* A = a.d_init_c2w + (size_t)16 * c;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                GR[3 * i + k] = G[4 * i] * A[4 * k] + G[4 * i + 1] * A[4 * k + 1] + G[4 * i + 2] * A[4 * k + 2]
                              + G[4 * i + 3] * A[4 * k + 3];
            gt[i] = G[4 * i] * A[12] + G[4 * i + 1] * A[13] + G[4 * i + 2] * A[14] + G[4 * i + 3] * A[15];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            GR[3 * i] = G[4 * i];
            GR[3 * i + 1] = G[4 * i + 1];
            GR[3 * i + 2] = G[4 * i + 2];
            gt[i] = G[4 * i + 3];
        }
    }
    if (a.d_g_t) {
        a.d_g_t[3 * c] = gt[0];
        a.d_g_t[3 * c + 1] = gt[1];
        a.d_g_t[3 * c + 2] = gt[2];
    }
    if (!a.d_g_r) return;

    // through R = I + al K + be K^2, K = skew(r), n = |r| + 1e-15 (d|r|/dr = r/|r|, 0 at r = 0 as torch's norm)
    const float r0 = a.d_r[3 * c], r1 = a.d_r[3 * c + 1], r2 = a.d_r[3 * c + 2];
    const float nr = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
    float al, be, dal, dbe;
    nfl_rodrigues_coeffs(nr + 1e-15f, al, be, dal, dbe);
    const float K[9] = {0.f, -r2, r1, r2, 0.f, -r0, -r1, r0, 0.f};
    float GK[9], s_k = 0.f, s_kk = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // (GR K^T + K^T GR)_ij
            float x = 0.f, kk = 0.f;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                x += GR[3 * i + m] * K[3 * j + m] + K[3 * m + i] * GR[3 * m + j];
                kk += K[3 * i + m] * K[3 * m + j];
            }
            GK[3 * i + j] = al * GR[3 * i + j] + be * x;
            s_k += GR[3 * i + j] * K[3 * i + j];
            s_kk += GR[3 * i + j] * kk;
        }
    float gr[3] = {GK[7] - GK[5], GK[2] - GK[6], GK[3] - GK[1]};
    if (nr > 0.f) {
        const float gn = (dal * s_k + dbe * s_kk) / nr;
        gr[0] += gn * r0;
        gr[1] += gn * r1;
        gr[2] += gn * r2;
    }
    a.d_g_r[3 * c] = gr[0];
    a.d_g_r[3 * c + 1] = gr[1];
    a.d_g_r[3 * c + 2] = gr[2];
}

int nfl_pose_check(const nfl_pose_args* a) {
    if (!a || a->n_cams < 0 || a->n_ids < 0 || a->n_rays < 0 || a->cam_stride < 5) return NFL_EINVAL;
    if (a->n_cams > 0 && (!a->d_r || !a->d_t)) return NFL_EINVAL;
    if (a->n_rays > 0 && (!a->d_row_of_id || !a->d_ts || !a->d_rays_cam || !a->d_rows)) return NFL_EINVAL;
    return NFL_OK;
}

}  // namespace

extern "C" int nfl_pose_rays(const nfl_pose_args* args, void* stream) {
    const int e = nfl_pose_check(args);
    if (e != NFL_OK) return e;
    if (args->n_rays == 0) return NFL_OK;
    if (!args->d_rays) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_pose_rays_kernel, dim3((args->n_rays + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}

extern "C" int nfl_pose_rays_backward(const nfl_pose_args* args, void* stream) {
    const int e = nfl_pose_check(args);
    if (e != NFL_OK) return e;
    if (args->n_rays > 0 && !args->d_g_rays) return NFL_EINVAL;
    if (args->n_cams == 0 || (!args->d_g_r && !args->d_g_t)) return NFL_OK;
    hipLaunchKernelGGL(nfl_pose_rays_bwd_kernel, dim3((args->n_cams + 3) / 4), dim3(256), 0,
                       static_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
