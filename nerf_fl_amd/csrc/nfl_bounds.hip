// nfl_bounds.hip -- per-image depth bounds of a sparse point cloud (include/nerf_fl_amd.h, "depth bounds"): what the
// reference does per image in a Python loop (datasets/phototourism.py:127-131: transform every point into the camera,
// keep those in front of it, np.percentile 0.1 / 99.9 of their depths) as ONE launch with no (image, point) intermediate.
//
// One workgroup per image.  The depth of a point is one fp64 dot product with the third row of the image's w2c, so the
// workgroup RECOMPUTES the depths from the point list (24 B per point, a few MB: it stays in L2) on every pass instead of
// storing them.  A positive double's bit pattern orders like the number, so the order statistics come from an exact MSB
// radix select over that 64-bit key: 8 passes of 8 bits, each a 256-bin histogram of the keys that still carry the
// selected prefix, built with integer LDS atomics.  numpy's `linear` percentile needs the order statistics floor(v) and
// floor(v) + 1 of the virtual index v = q (m - 1), so four ranks are selected together; ranks whose prefixes still agree
// share one histogram (both of a percentile usually do to the last passes, and all four do in the first two), so a point
// costs one LDS atomic in the passes where most points still match.
//
// 1024 threads = 4 histograms x 256 bins: after a pass, thread t owns bin t & 255 of histogram t >> 8, the four
// histograms are scanned at once (wave scan by __shfl_up, 4 wave totals per histogram), and the one thread whose bin
// holds a rank appends its digit to that rank's prefix.  LDS: 4 KB of histograms; nothing is written to global memory
// but the 2 results and the count per image, by one thread, with plain stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nerf_fl_amd.h"

#define NB_THREADS 1024
#define NB_BINS 256
#define NB_RANKS 4
// a prefix no key matches: keys are positive doubles, their bit 63 is clear, and a pass compares bits 63 .. shift + 8
#define NB_NO_PREFIX 0xFFFFFFFFFFFFFFFFull

// (xyz_h @ w2c.T)[:, 2] of phototourism.py:128 for one point, every operation rounded on its own (-ffp-contract=off)
__device__ __forceinline__ double nb_depth(const double* __restrict__ xyz, int i, double r0, double r1, double r2, double t) {
    const double* p = xyz + 3 * (size_t)i;
    return ((p[0] * r0 + p[1] * r1) + p[2] * r2) + t;
}

// virtual index q (m - 1) of numpy's `linear` method: lower order statistic, upper one (clipped), interpolation weight
__device__ __forceinline__ void nb_rank(double q, uint32_t m, uint32_t& lo, uint32_t& hi, double& gamma) {
    const double v = q * (double)(m - 1);
    double f = floor(v);
    if (!(f >= 0.0)) f = 0.0;
    if (f > (double)(m - 1)) f = (double)(m - 1);
    lo = (uint32_t)f;
    hi = lo + 1 < m ? lo + 1 : m - 1;
    gamma = v - f;
}

// numpy's _lerp: a + (b - a) t, taken from the other end for t >= 0.5
__device__ __forceinline__ double nb_lerp(double a, double b, double t) {
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

__global__ __launch_bounds__(NB_THREADS) void nfl_bounds_kernel(const nfl_bounds_args a) {
    __shared__ uint32_t hist[NB_RANKS][NB_BINS];
    __shared__ uint32_t wave_total[NB_RANKS][4];
    __shared__ uint64_t s_prefix[NB_RANKS];
    __shared__ uint32_t s_rank[NB_RANKS];

    const int img = blockIdx.x, tid = threadIdx.x, n = a.n_points;
    const int sd = tid >> 8, sb = tid & 255, sw = (tid >> 6) & 3, lane = tid & 63;      // this thread's histogram bin
    const double r0 = a.d_row[4 * (size_t)img], r1 = a.d_row[4 * (size_t)img + 1], r2 = a.d_row[4 * (size_t)img + 2],
                 rt = a.d_row[4 * (size_t)img + 3];
    uint32_t m = 0;

    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        // the ranks' state, and one histogram per distinct prefix (all uniform over the workgroup)
        uint64_t pf[NB_RANKS], up[NB_RANKS];
        uint32_t rk[NB_RANKS];
        int slot[NB_RANKS], nd = 0;
#pragma unroll
        for (int s = 0; s < NB_RANKS; ++s) {
            pf[s] = pass ? s_prefix[s] : 0;
            rk[s] = pass ? s_rank[s] : 0;
            up[s] = NB_NO_PREFIX;
        }
#pragma unroll
        for (int s = 0; s < NB_RANKS; ++s) {
            int f = -1;
#pragma unroll
            for (int s2 = 0; s2 < s; ++s2)
                if (f < 0 && pf[s2] == pf[s]) f = slot[s2];
            if (f < 0) {
                f = nd++;
#pragma unroll
                for (int d = 0; d < NB_RANKS; ++d)
                    if (d == f) up[d] = pf[s];
            }
            slot[s] = f;
        }
        hist[sd][sb] = 0;
        __syncthreads();

        if (pass == 0) {
            // every point in front of the camera counts; nearly all share the top digit (sign and 7 exponent bits), so
            // a thread adds a run of equal digits with one atomic
            uint32_t run_digit = 0, run = 0;
#pragma unroll 4
            for (int i = tid; i < n; i += NB_THREADS) {
                const double z = nb_depth(a.d_xyz, i, r0, r1, r2, rt);
                if (z > 0.0) {
                    const uint32_t digit = (uint32_t)((uint64_t)__double_as_longlong(z) >> 56);
                    if (digit != run_digit) {
                        if (run) atomicAdd(&hist[0][run_digit], run);
                        run_digit = digit;
                        run = 0;
                    }
                    ++run;
                }
            }
            if (run) atomicAdd(&hist[0][run_digit], run);
        } else {
#pragma unroll 4
            for (int i = tid; i < n; i += NB_THREADS) {
                const double z = nb_depth(a.d_xyz, i, r0, r1, r2, rt);
                if (z > 0.0) {
                    const uint64_t key = (uint64_t)__double_as_longlong(z);
                    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
#pragma unroll
                    for (int d = 0; d < NB_RANKS; ++d)
                        if (((key ^ up[d]) >> (shift + 8)) == 0) atomicAdd(&hist[d][digit], 1u);
                }
            }
        }
        __syncthreads();

        // inclusive scan of the four histograms at once
        const uint32_t c = hist[sd][sb];
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_total[sd][sw] = incl;
        __syncthreads();
        for (int w = 0; w < sw; ++w) incl += wave_total[sd][w];

        if (pass == 0) {
            m = wave_total[0][0] + wave_total[0][1] + wave_total[0][2] + wave_total[0][3];
            if (m == 0) {                                   // nothing in front of this camera (uniform: all threads leave)
                if (tid == 0) {
                    a.d_count[img] = 0;
                    a.d_bounds[img] = a.d_bounds[(size_t)a.n_images + img] = __longlong_as_double(0x7FF8000000000000ll);
                }
                return;
            }
            double g;
            nb_rank(a.q_lo, m, rk[0], rk[1], g);
            nb_rank(a.q_hi, m, rk[2], rk[3], g);
        }
        // the bin that holds a rank: excl <= rank < incl (exactly one thread per rank, in that rank's histogram)
        const uint32_t excl = incl - c;
#pragma unroll
        for (int s = 0; s < NB_RANKS; ++s)
            if (slot[s] == sd && excl <= rk[s] && rk[s] < incl) {
                s_prefix[s] = pf[s] | ((uint64_t)sb << shift);
                s_rank[s] = rk[s] - excl;
            }
        __syncthreads();
    }

    if (tid == 0) {
        uint32_t lo, hi;
        double g;
        a.d_count[img] = (int32_t)m;
        nb_rank(a.q_lo, m, lo, hi, g);
        a.d_bounds[img] = nb_lerp(__longlong_as_double((long long)s_prefix[0]), __longlong_as_double((long long)s_prefix[1]), g);
        nb_rank(a.q_hi, m, lo, hi, g);
        a.d_bounds[(size_t)a.n_images + img] =
            nb_lerp(__longlong_as_double((long long)s_prefix[2]), __longlong_as_double((long long)s_prefix[3]), g);
    }
}

extern "C" int nfl_depth_bounds(const nfl_bounds_args* args, void* stream) {
    if (!args || !args->d_xyz || !args->d_row || !args->d_bounds || !args->d_count) return NFL_EINVAL;
    if (args->n_points < 1 || args->n_points > (1 << 30) || args->n_images < 1) return NFL_EINVAL;
    if (!(args->q_lo >= 0.0 && args->q_lo <= 1.0 && args->q_hi >= 0.0 && args->q_hi <= 1.0)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_bounds_kernel, dim3(args->n_images), dim3(NB_THREADS), 0, static_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
