// nfl_gather.hip -- a training batch straight from uint8 images kept on the device (include/nerf_fl_amd.h,
// "training batches from uint8 images"): replaces the reference's all_rays / all_rgbs buffers (datasets/blender.py:73-101,
// datasets/phototourism.py:150-183; 52 B per pixel), the epoch's randperm (8 B per pixel) and the three index gathers of a
// step by ONE launch that reads 3 or 4 B per pixel.
//
// One thread per output row.  The row's flat pixel comes from a keyed Feistel permutation that is computed, not stored;
// its image from a binary search of the records' pixel prefix (ceil(log2 n_images) dependent loads of a table that is
// at most 1500 x 104 B and stays in L2; a batch touches it from 4 .. 16 workgroups); its ray from nfl_cam_ray, the device
// function behind nfl_gen_rays and the render kernels' camera prologue, so that all three give the same bits.  The kernel
// moves 52 B per ray out and at most one cache line per ray in: it is bound by launch and load latency, not by bandwidth.
// A world row is two 16-byte stores; a camera row (20 B) and a colour row (12 B) are not 16-byte aligned and go out as
// dwords, which the write-combining L2 merges (rows are consecutive per lane).
#include "nfl_math.h"
#include "nfl_pixel.h"

#define NFL_PERM_ROUNDS 6

struct NflPerm {
    uint32_t k[NFL_PERM_ROUNDS];   // round keys (host: splitmix64 of the key)
    int h;                         // bits of a half
};

NFL_DEV uint32_t nfl_perm_mix(uint32_t v) {      // murmur3's 32-bit finaliser
    v ^= v >> 16;
    v *= 0x85EBCA6Bu;
    v ^= v >> 13;
    v *= 0xC2B2AE35u;
    v ^= v >> 16;
    return v;
}

// a bijection of [0, n): Feistel over [0, 4^h) >= n, walked along its cycle until it lands below n again (the cycle
// through x < n returns to x, so the walk ends)
NFL_DEV long long nfl_perm(const NflPerm& pk, long long n, long long x) {
    const uint32_t mask = (1u << pk.h) - 1u;
    do {
        uint32_t l = (uint32_t)(x >> pk.h), r = (uint32_t)x & mask;
#pragma unroll
        for (int i = 0; i < NFL_PERM_ROUNDS; ++i) {
            const uint32_t t = l ^ (nfl_perm_mix(r * 0x9E3779B1u + pk.k[i]) & mask);
            l = r;
            r = t;
        }
        x = ((long long)l << pk.h) | r;
    } while (x >= n);
    return x;
}

__global__ __launch_bounds__(256) void nfl_gather_kernel(const nfl_gather_args a, const NflPerm pk, const int permute) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= a.count) return;
    const long long p = a.start + row;
    const long long q = permute ? nfl_perm(pk, a.n_pixels, p) : p;      // in [0, n_pixels) (host-checked range)
    // last image whose prefix is <= q
    int lo = 0, hi = a.n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.d_table[mid].pix0 <= q) lo = mid; else hi = mid - 1;
    }
    const nfl_image_rec& im = a.d_table[lo];
    const long long local = q - im.pix0;                                 // pixel of the image, row-major
    if (a.d_rays) {
        if (a.layout == NFL_LAYOUT_WORLD) {
            f4v r0, r1;
            nfl_cam_ray(im, local, r0, r1);
            f4v* o = reinterpret_cast<f4v*>(a.d_rays + (size_t)row * 8);
            o[0] = r0;
            o[1] = r1;
        } else {
            const float i = (float)(local % im.width), j = (float)(local / im.width);
            float* o = a.d_rays + (size_t)row * 5;
            o[0] = (i - im.cx) / im.fx;
            o[1] = -(j - im.cy) / im.fy;
            o[2] = -1.f;
            o[3] = im.near;
            o[4] = im.far;
        }
    }
    if (a.d_ts) a.d_ts[row] = im.id;
    if (a.d_rgb) {
        float c[3];
        nfl_pixel_rgb(a.d_pixels, im, local, c);      // nfl_pixel.h: shared with nfl_image_metrics
        float* o = a.d_rgb + (size_t)row * 3;
        o[0] = c[0];
        o[1] = c[1];
        o[2] = c[2];
    }
}

extern "C" int nfl_gather_batch(const nfl_gather_args* args, void* stream) {
    if (!args || !args->d_pixels || !args->d_table || args->n_images < 1) return NFL_EINVAL;
    if (args->n_pixels < 1 || args->n_pixels >= (1LL << 40) || args->start < 0 || args->count < 0) return NFL_EINVAL;
    if (args->start + (int64_t)args->count > args->n_pixels) return NFL_EINVAL;
    if (args->layout != NFL_LAYOUT_WORLD && args->layout != NFL_LAYOUT_CAMERA) return NFL_EINVAL;
    if (args->count == 0 || (!args->d_rays && !args->d_ts && !args->d_rgb)) return NFL_OK;
    NflPerm pk;
    int bits = 0;
    while (bits < 40 && (1LL << bits) < args->n_pixels) ++bits;          // bits(n - 1)
    pk.h = bits <= 2 ? 1 : (bits + 1) / 2;
    uint64_t state = args->key;
    for (int i = 0; i < NFL_PERM_ROUNDS; ++i) {                           // splitmix64
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        pk.k[i] = (uint32_t)(z ^ (z >> 31));
    }
    hipLaunchKernelGGL(nfl_gather_kernel, dim3((args->count + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *args, pk, args->key != 0 ? 1 : 0);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
