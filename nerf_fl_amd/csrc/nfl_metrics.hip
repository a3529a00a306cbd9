// nfl_metrics.hip -- score a rendered image against its ground truth where both lie (include/nerf_fl_amd.h, "scoring a
// rendered image"): squared error, masked squared error and the 3 x 3 Gaussian SSIM of the reference's metrics.py in one
// pass over the prediction (fp32) and the uint8 image of an image bank (or an fp32 target), plus the depth image of
// utils/visualization.py.  A split is scored into one small fp64 table: no per-image host sync, nothing that grows with it.
//
// nfl_metrics_tiles_kernel: one 256-thread workgroup per tile of 64 columns x 16 rows of the region.  The tile and its
// one-pixel halo (reflected at the REGION's border) are staged in LDS as fp32 after conversion and clipping: 6 colour
// planes and the valid flag, rows of 66 floats, so the three taps a lane reads sit on consecutive banks.  A wavefront then
// owns 64 columns x 4 rows: every lane filters its column's 6 halo rows horizontally for the 5 moments of each channel
// (p, t, pp, tt, pt) and combines three of them vertically per output pixel -- the 3 x 3 window is an outer product.
// Sums are kept per lane in fp64 (12 elements each), reduced across the wavefront by shuffles and across the 4 wavefronts
// in a fixed order; the workgroup writes ONE partial.  nfl_metrics_finish_kernel (one workgroup) adds the partials in the
// fixed order of nfl_reduce.h and writes the slot.  Nothing is atomic, memset or copied: two runs give the same bits and the pair of
// launches can be captured in a HIP graph.  The work is launch-bound (10 MB at 800 x 800), as nfl_gather_batch is.
#include <math.h>

#include "nfl_pixel.h"
#include "nfl_reduce.h"

#define NFL_MT_W 64
#define NFL_MT_H 16
#define NFL_MT_LD (NFL_MT_W + 2)
#define NFL_MT_PART 5                 // doubles per partial: sse, count, sse_valid, count_valid, ssim_sum
#define NFL_DEPTH_MAX_PARTS 256

// the normalised window, g = exp(-(k - 1)^2 / 4.5) / sum: computed in fp64, rounded once
#define NFL_SSIM_G0 0.30780132912346997f
#define NFL_SSIM_G1 0.38439734175306f
#define NFL_SSIM_C1 1e-4f
#define NFL_SSIM_C2 9e-4f

// one 3-tap correlation: the two equal outer taps are added first, then one multiply and one fused multiply-add (three
// roundings; the translation unit is built with -ffp-contract=off, so this is the only fused operation of the filter)
NFL_DEV float nfl_tap3(float a, float b, float c) { return fmaf(NFL_SSIM_G0, a + c, NFL_SSIM_G1 * b); }

NFL_DEV int nfl_reflect(int i, int n) { return i < 0 ? 1 : (i >= n ? n - 2 : i); }      // i in [-1, n], n >= 2

NFL_DEV double nfl_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                                                             // lane 0 holds the sum
}

__global__ __launch_bounds__(256) void nfl_metrics_tiles_kernel(const nfl_metrics_args a) {
    __shared__ float s[7][NFL_MT_H + 2][NFL_MT_LD];
    __shared__ double red[4][NFL_MT_PART];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = a.x1 - a.x0, h = a.y1 - a.y0;
    const int tx0 = blockIdx.x * NFL_MT_W, ty0 = blockIdx.y * NFL_MT_H;
    const bool bank = a.d_pixels != nullptr;
    nfl_image_rec im;
    bool bad = false;
    if (bank) {
        im = a.d_table[a.image];
        bad = im.width != a.width || im.height != a.height || (im.channels != 3 && im.channels != 4);
    }
    for (int idx = tid; idx < (NFL_MT_H + 2) * NFL_MT_LD; idx += 256) {
        const int r = idx / NFL_MT_LD, c = idx - r * NFL_MT_LD;
        int ry = ty0 + r - 1, rx = tx0 + c - 1;                     // region coordinates, halo included
        float p[3] = {0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f}, valid = 0.f;
        if (!bad && ry <= h && rx <= w) {
            ry = nfl_reflect(ry, h);
            rx = nfl_reflect(rx, w);
            const long long pix = (long long)(a.y0 + ry) * a.width + (a.x0 + rx);      // < height * width < 2^31
            const float* src = a.d_pred + pix * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float v = src[k];
                p[k] = a.clip ? (v < 0.f ? 0.f : (v > 1.f ? 1.f : v)) : v;             // NaN stays NaN (torch.clamp)
            }
            if (bank) {
                valid = nfl_pixel_rgb(a.d_pixels, im, pix, t) > 0u ? 1.f : 0.f;
            } else {
                const float* g = a.d_target + pix * 3;
                t[0] = g[0];
                t[1] = g[1];
                t[2] = g[2];
                valid = (!a.d_mask || a.d_mask[pix]) ? 1.f : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s[k][r][c] = p[k];
            s[3 + k][r][c] = t[k];
        }
        s[6][r][c] = valid;
    }
    __syncthreads();

    double sse = 0.0, sse_valid = 0.0, ssim_sum = 0.0, count = 0.0, count_valid = 0.0;
    const int rx = tx0 + lane, r0 = wave * 4;
    if (rx < w && ty0 + r0 < h) {
        float hz[6][15];                                            // horizontally filtered moments of the 6 halo rows
#pragma unroll
        for (int j = 0; j < 6; ++j) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float pl = s[k][r0 + j][lane], pc = s[k][r0 + j][lane + 1], pr = s[k][r0 + j][lane + 2];
                const float tl = s[3 + k][r0 + j][lane], tc = s[3 + k][r0 + j][lane + 1], tr = s[3 + k][r0 + j][lane + 2];
                hz[j][5 * k + 0] = nfl_tap3(pl, pc, pr);
                hz[j][5 * k + 1] = nfl_tap3(tl, tc, tr);
                hz[j][5 * k + 2] = nfl_tap3(pl * pl, pc * pc, pr * pr);
                hz[j][5 * k + 3] = nfl_tap3(tl * tl, tc * tc, tr * tr);
                hz[j][5 * k + 4] = nfl_tap3(pl * tl, pc * tc, pr * tr);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ry = ty0 + r0 + i;
            if (ry >= h) break;
            const size_t o = ((size_t)ry * w + rx) * 3;
            const bool valid = s[6][r0 + i + 1][lane + 1] != 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float p = s[k][r0 + i + 1][lane + 1], t = s[3 + k][r0 + i + 1][lane + 1];
                const double d = (double)p - (double)t, d2 = d * d;
                sse += d2;
                count += 1.0;
                if (valid) {
                    sse_valid += d2;
                    count_valid += 1.0;
                }
                const float mu1 = nfl_tap3(hz[i][5 * k + 0], hz[i + 1][5 * k + 0], hz[i + 2][5 * k + 0]);
                const float mu2 = nfl_tap3(hz[i][5 * k + 1], hz[i + 1][5 * k + 1], hz[i + 2][5 * k + 1]);
                const float e11 = nfl_tap3(hz[i][5 * k + 2], hz[i + 1][5 * k + 2], hz[i + 2][5 * k + 2]);
                const float e22 = nfl_tap3(hz[i][5 * k + 3], hz[i + 1][5 * k + 3], hz[i + 2][5 * k + 3]);
                const float e12 = nfl_tap3(hz[i][5 * k + 4], hz[i + 1][5 * k + 4], hz[i + 2][5 * k + 4]);
                const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
                const float s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
                const float S = ((2.f * m12 + NFL_SSIM_C1) * (2.f * s12 + NFL_SSIM_C2))
                                / ((m11 + m22 + NFL_SSIM_C1) * (s1 + s2 + NFL_SSIM_C2));
                float loss = 1.f - S;
                loss = loss < 0.f ? 0.f : (loss > 1.f ? 1.f : loss);
                const float m = 1.f - loss;
                ssim_sum += (double)m;
                if (a.d_ssim_map) a.d_ssim_map[o + k] = m;
                if (a.d_pred_u8) {
                    const float q = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);
                    a.d_pred_u8[o + k] = (uint8_t)(q * 255.0f);
                }
            }
        }
    }
    double part[NFL_MT_PART] = {sse, count, sse_valid, count_valid, ssim_sum};
#pragma unroll
    for (int k = 0; k < NFL_MT_PART; ++k) {
        const double v = nfl_wave_sum(part[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < NFL_MT_PART) {
        double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        if (bad) v = nan("");
        static_cast<double*>(a.d_scratch)[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * NFL_MT_PART + tid] = v;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in index order, then the library's fold of the 256 threads (nfl_reduce.h)
__global__ __launch_bounds__(256) void nfl_metrics_finish_kernel(const double* __restrict__ parts, int n_parts,
                                                                 double* __restrict__ row) {
    __shared__ double lds[NFL_MT_PART * 128];
    const int tid = threadIdx.x;
    double acc[NFL_MT_PART] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n_parts; i += 256) {
#pragma unroll
        for (int k = 0; k < NFL_MT_PART; ++k) acc[k] += parts[(size_t)i * NFL_MT_PART + k];
    }
    ng_fold<NFL_MT_PART>(acc, lds, NgAdd());
    if (tid == 0) {
        const double sse = acc[0], count = acc[1], sse_valid = acc[2], count_valid = acc[3], ssim_sum = acc[4];
        row[NFL_METRIC_SSE] = sse;
        row[NFL_METRIC_COUNT] = count;
        row[NFL_METRIC_SSE_VALID] = sse_valid;
        row[NFL_METRIC_COUNT_VALID] = count_valid;
        row[NFL_METRIC_SSIM_SUM] = ssim_sum;
        row[NFL_METRIC_PSNR] = -10.0 * log10(sse / count);
        row[NFL_METRIC_PSNR_VALID] = -10.0 * log10(sse_valid / count_valid);
        row[NFL_METRIC_SSIM] = ssim_sum / count;
    }
}

static long long nfl_metrics_tiles(int h, int w) {
    return (long long)((w + NFL_MT_W - 1) / NFL_MT_W) * ((h + NFL_MT_H - 1) / NFL_MT_H);
}

// 0: a non-empty region inside the image; 1: an empty one; -1: bad
static int nfl_region_check(int width, int height, int x0, int x1, int y0, int y1) {
    if (width < 1 || height < 1 || (long long)width * height >= (1LL << 31)) return -1;
    if (x0 < 0 || y0 < 0 || x1 < x0 || y1 < y0 || x1 > width || y1 > height) return -1;
    return (x1 == x0 || y1 == y0) ? 1 : 0;
}

extern "C" size_t nfl_image_metrics_scratch_bytes(int32_t h, int32_t w) {
    if (h < 1 || w < 1) return 0;
    return (size_t)nfl_metrics_tiles(h, w) * NFL_MT_PART * sizeof(double);
}

extern "C" int nfl_image_metrics(const nfl_metrics_args* a, void* stream) {
    if (!a || !a->d_pred || !a->d_results || !a->d_scratch) return NFL_EINVAL;
    const bool bank = a->d_pixels || a->d_table, tensor = a->d_target != nullptr;
    if (bank == tensor || (bank && (!a->d_pixels || !a->d_table)) || (a->d_mask && !tensor)) return NFL_EINVAL;
    if (bank && (a->n_images < 1 || a->image < 0 || a->image >= a->n_images)) return NFL_EINVAL;
    if (a->n_slots < 1 || a->slot < 0 || a->slot >= a->n_slots) return NFL_EINVAL;
    if (((uintptr_t)a->d_scratch & 7u) || ((uintptr_t)a->d_results & 7u)) return NFL_EINVAL;
    const int rc = nfl_region_check(a->width, a->height, a->x0, a->x1, a->y0, a->y1);
    if (rc < 0) return NFL_EINVAL;
    if (rc == 1) return NFL_OK;
    const int w = a->x1 - a->x0, h = a->y1 - a->y0;
    if (w < 2 || h < 2) return NFL_EINVAL;                                   // reflection needs two pixels
    if (a->scratch_bytes < nfl_image_metrics_scratch_bytes(h, w)) return NFL_EINVAL;
    const dim3 grid((w + NFL_MT_W - 1) / NFL_MT_W, (h + NFL_MT_H - 1) / NFL_MT_H);
    if (grid.y > 65535u) return NFL_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nfl_metrics_tiles_kernel, grid, dim3(256), 0, st, *a);
    hipLaunchKernelGGL(nfl_metrics_finish_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(a->d_scratch),
                       (int)(grid.x * grid.y), a->d_results + (size_t)a->slot * NFL_METRIC_COLUMNS);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}

// ---- depth image (utils/visualization.py:10-15) ------------------------------------------------------------------------
// np.nan_to_num: NaN -> 0, +-inf -> +-FLT_MAX
NFL_DEV float nfl_depth_value(const nfl_depth_args& a, int idx, int w) {
    const int y = idx / w, x = idx - y * w;
    const float d = a.d_depth[(size_t)(a.y0 + y) * a.width + (a.x0 + x)];
    if (d != d) return 0.f;
    return d > 3.402823466e38f ? 3.402823466e38f : (d < -3.402823466e38f ? -3.402823466e38f : d);
}

NFL_DEV void nfl_block_minmax(float& mi, float& ma, float (*red)[256]) {
    const int tid = threadIdx.x;
    red[0][tid] = mi;
    red[1][tid] = ma;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] = fminf(red[0][tid], red[0][tid + off]);
            red[1][tid] = fmaxf(red[1][tid], red[1][tid + off]);
        }
        __syncthreads();
    }
    mi = red[0][0];
    ma = red[1][0];
}

__global__ __launch_bounds__(256) void nfl_depth_minmax_kernel(const nfl_depth_args a) {
    __shared__ float red[2][256];
    const int w = a.x1 - a.x0, n = w * (a.y1 - a.y0);
    float mi = INFINITY, ma = -INFINITY;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
        const float d = nfl_depth_value(a, idx, w);
        mi = fminf(mi, d);
        ma = fmaxf(ma, d);
    }
    nfl_block_minmax(mi, ma, red);
    if (threadIdx.x == 0) {
        float* o = static_cast<float*>(a.d_scratch) + 2 * blockIdx.x;
        o[0] = mi;
        o[1] = ma;
    }
}

__global__ __launch_bounds__(256) void nfl_depth_image_kernel(const nfl_depth_args a, const int n_parts) {
    __shared__ float red[2][256];
    const int tid = threadIdx.x, w = a.x1 - a.x0, n = w * (a.y1 - a.y0);
    const float* parts = static_cast<const float*>(a.d_scratch);
    float mi = tid < n_parts ? parts[2 * tid] : INFINITY, ma = tid < n_parts ? parts[2 * tid + 1] : -INFINITY;
    nfl_block_minmax(mi, ma, red);                       // every workgroup: at most 256 partials, minima are exact
    const int idx = blockIdx.x * 256 + tid;
    if (idx >= n) return;
    const float x = (nfl_depth_value(a, idx, w) - mi) / (ma - mi + 1e-8f);
    const float v = 255.f * x;
    const uint32_t level = v >= 0.f ? (v < 255.f ? (uint32_t)v : 255u) : 0u;       // x is in [0, 1]; a NaN (inf / inf) -> 0
    uint8_t* o = a.d_image + (size_t)idx * 3;
    if (a.d_lut) {
        o[0] = a.d_lut[3 * level];
        o[1] = a.d_lut[3 * level + 1];
        o[2] = a.d_lut[3 * level + 2];
    } else {
        o[0] = o[1] = o[2] = (uint8_t)level;
    }
}

static int nfl_depth_parts(int h, int w) {
    const long long blocks = ((long long)h * w + 255) / 256;
    return (int)(blocks < NFL_DEPTH_MAX_PARTS ? blocks : NFL_DEPTH_MAX_PARTS);
}

extern "C" size_t nfl_depth_image_scratch_bytes(int32_t h, int32_t w) {
    if (h < 1 || w < 1) return 0;
    return (size_t)nfl_depth_parts(h, w) * 2 * sizeof(float);
}

extern "C" int nfl_depth_image(const nfl_depth_args* a, void* stream) {
    if (!a || !a->d_depth || !a->d_image || !a->d_scratch || ((uintptr_t)a->d_scratch & 3u)) return NFL_EINVAL;
    const int rc = nfl_region_check(a->width, a->height, a->x0, a->x1, a->y0, a->y1);
    if (rc < 0) return NFL_EINVAL;
    if (rc == 1) return NFL_OK;
    const int w = a->x1 - a->x0, h = a->y1 - a->y0;
    if (a->scratch_bytes < nfl_depth_image_scratch_bytes(h, w)) return NFL_EINVAL;
    const int parts = nfl_depth_parts(h, w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nfl_depth_minmax_kernel, dim3(parts), dim3(256), 0, st, *a);
    hipLaunchKernelGGL(nfl_depth_image_kernel, dim3((unsigned)(((long long)h * w + 255) / 256)), dim3(256), 0, st, *a, parts);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
