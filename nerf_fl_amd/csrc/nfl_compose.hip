// nfl_compose.hip -- the small fp32 products of the composition through xyz_encoding_final (nfl_compose.h), one launch:
// the kernel, its launcher, and the forward re-pack's fold.  What the tasks are is host code: nfl_compose.cpp.
// The operands are the fp32 master weights and the finished (unscaled) G / bias gradients; everything is L2-resident.
#include <hip/hip_runtime.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_compose.h"
#include "nfl_macros.h"

typedef float wg_f4 __attribute__((ext_vector_type(4)));

// One 32 x 32 output tile per workgroup on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact products, fp32
// accumulation): the four waves split K, every lane fetches its operands straight from global memory (float4 along k where
// k is the contiguous index, one dword per k otherwise; all loads of a wave are in flight before its first MFMA), the
// partial tiles meet in LDS.  MFMA j of a wave takes, in lane half h, k = k_wave + 8 (j / 4) + 4 h + (j % 4): any pairing
// of the two k of a step is as good as another as long as A and B agree.  (The first version staged 32 x 128 operand
// blocks through LDS for scalar FMAs and was LDS-bound: 20-30 us; this one is one memory round trip and 16-32 MFMAs per wave.)
template <int NJ>       // MFMAs per wave = (K / 4) / 2
__device__ __forceinline__ void wg_compose_pass(f16v& acc, const float* A, int sam, int sak, const float* B, int sbk, int sbn,
                                                int m, int n, bool n_ok, int k_wave, int h, bool avec, bool bvec) {
    float ra[NJ], rb[NJ];
#pragma unroll
    for (int g = 0; g < NJ / 4; ++g) {
        const int kq = k_wave + 8 * g + 4 * h;
        if (sak == 1 && avec) {
            const wg_f4 v = *reinterpret_cast<const wg_f4*>(A + (size_t)m * sam + kq);
            ra[4 * g] = v[0]; ra[4 * g + 1] = v[1]; ra[4 * g + 2] = v[2]; ra[4 * g + 3] = v[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) ra[4 * g + e] = A[(size_t)m * sam + (size_t)(kq + e) * sak];
        }
        if (!n_ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) rb[4 * g + e] = 0.f;
        } else if (sbk == 1 && sbn != 1 && bvec) {
            const wg_f4 v = *reinterpret_cast<const wg_f4*>(B + (size_t)n * sbn + kq);
            rb[4 * g] = v[0]; rb[4 * g + 1] = v[1]; rb[4 * g + 2] = v[2]; rb[4 * g + 3] = v[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) rb[4 * g + e] = B[(size_t)(kq + e) * sbk + (size_t)n * sbn];
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[j], rb[j], acc, 0, 0, 0);
}

__global__ __launch_bounds__(256) void nfl_wgrad_compose_kernel(const WgCompose Cc) {
    __shared__ float red[4][16][64];
    int ti = 0;
    while (ti + 1 < Cc.n_tasks && (int)blockIdx.x >= Cc.t[ti + 1].tile0) ++ti;
    const WgGemm& T = Cc.t[ti];
    const int tile = blockIdx.x - T.tile0, m0 = 32 * (tile / T.tiles_n), n0 = 32 * (tile % T.tiles_n);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const int m = m0 + (lane & 31), n = n0 + (lane & 31);      // M is a multiple of 32 (256 or 128); N is 256 or 1
    const bool n_ok = n < T.N;
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // K and K2 are 128 or 256 (host-checked: wg_check of nfl_compose.cpp, as is M above): 32 or 64 per wave
    if (T.K == 256) wg_compose_pass<32>(acc, T.A, T.sam, T.sak, T.B, T.sbk, T.sbn, m, n, n_ok, 64 * wave, h, T.avec, T.bvec);
    else wg_compose_pass<16>(acc, T.A, T.sam, T.sak, T.B, T.sbk, T.sbn, m, n, n_ok, 32 * wave, h, T.avec, T.bvec);
    if (T.K2 == 256) wg_compose_pass<32>(acc, T.A2, T.sam2, T.sak2, T.B2, T.sbk2, T.sbn2, m, n, n_ok, 64 * wave, h, T.avec, T.bvec);
    else if (T.K2 == 128) wg_compose_pass<16>(acc, T.A2, T.sam2, T.sak2, T.B2, T.sbk2, T.sbn2, m, n, n_ok, 32 * wave, h, T.avec, T.bvec);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 4 * wave + q;                             // accumulator register r: row 8 (r / 4) + 4 h + (r % 4), column lane % 32
        const float c = red[0][r][lane] + red[1][r][lane] + red[2][r][lane] + red[3][r][lane];
        const int row = m0 + 8 * (r >> 2) + 4 * h + (r & 3);
        if (n_ok) T.Cp[(size_t)row * T.ldc + n] = (T.u ? __builtin_fmaf(T.u[row], T.v[n], c) : c) + (T.addm ? T.addm[row] : 0.f);
    }
}

// a task list that one of the builders of nfl_compose.cpp made and checked
void nfl_compose_launch(const WgCompose& Cc, hipStream_t s) {
    hipLaunchKernelGGL(nfl_wgrad_compose_kernel, dim3(Cc.n_wg), dim3(256), 0, s, Cc);
}

// Fold xyz_encoding_final into the layers that read its output, for the PACKED streams only (the parameters stay what
// they are): W_dir' = [W_dir[:, :256] W_fin | W_dir[:, 256:]], b_dir' = b_dir + W_dir[:, :256] b_fin, likewise for
// transient_encoding.0.  The caller hands in copies of W_dir / W_t0 (the side columns are kept, the first 256 columns
// overwritten) and receives the folded biases; nfl_pack_field(s) is then given these in place of the originals, and
// the streams carry no tiles for xyz_encoding_final (nfl_plan.cpp): one 256 x 256 layer less in the forward and in dgrad.
extern "C" int nfl_compose_forward(const nfl_field_params* params, int32_t has_t, int32_t n_side, int32_t n_tau,
                                   float* d_wdir_c, float* d_bdir_c, float* d_wt0_c, float* d_bt0_c, void* stream) {
    WgCompose Cc;
    const int rc = nfl_compose_forward_tasks(params, has_t, n_side, n_tau, d_wdir_c, d_bdir_c, d_wt0_c, d_bt0_c, &Cc);
    if (rc != NFL_OK) return rc;
    nfl_compose_launch(Cc, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
