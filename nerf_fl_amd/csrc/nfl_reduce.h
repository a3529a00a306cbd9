// nfl_reduce.h -- the library's fixed-order fp64 reduction of n elements to one row of columns, written ONCE: the mesh
// distance (nfl_meshdist_reduce), the registration (nfl_register_moments) and the finish of nfl_image_metrics add in this
// order, and tests/meshdist_ref.py and tests/registration_ref.py restate it.  DESIGN.md section 35.
//
//   parts    workgroup g of G, thread t of 256: elements g * 256 + t, + G * 256, ... in index order into the thread's columns
//            (registers); the 256 threads folded by halving (ng_fold); thread 0 writes the workgroup's partial row
//   finish   one workgroup: thread t combines partial rows t, t + 256, ... in index order, the same fold, thread 0 writes the row
//
// Nothing is atomic, so two runs give the same bits.  A reduction is a policy struct P, passed to the parts kernel by value:
//   P::cols                     columns a thread keeps
//   P::width                    doubles of a row, in the partials and in the result
//   P::column(k)                where the thread's column k lies in a row; increasing in k.  A place of the row that is no
//                               column's is left alone in the partials and written as zero in the result
//   P::Combine()(k, a, b)       two partial values of column k: NgAdd, or a functor of the policy's own
//   p.add(i, acc)               element i into the thread's columns
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NG_REDUCE_THREADS 256

struct NgAdd {
    __device__ __forceinline__ double operator()(int, double a, double b) const { return a + b; }
};

// The 256 threads' columns folded by halving into thread 0's: row t = combine(row t, row t + off) for t < off, off = 128 .. 1.
// The two steps that cross waves go through `lds`, NC x 128 doubles of it (128 rows, then 64); the six steps inside wave 0
// are cross-lane moves: lane t takes what lane t + off holds, which is what row t = combine(row t, row t + off) says, and
// lanes >= off then hold what nobody reads.  All 256 rows in LDS would be twice as much: 76 KiB for the registration's 38
// columns, half of the CU's 160 KiB for one workgroup.  Every thread of the workgroup calls; whoever used lds before is
// waited for.
template <int NC, typename Combine>
__device__ __forceinline__ void ng_fold(double* acc, double* lds, Combine combine) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid >= 128) {
#pragma unroll
        for (int k = 0; k < NC; ++k) lds[k * 128 + (tid - 128)] = acc[k];
    }
    __syncthreads();
    if (tid < 128) {
#pragma unroll
        for (int k = 0; k < NC; ++k) acc[k] = combine(k, acc[k], lds[k * 128 + tid]);
    }
    __syncthreads();
    if (tid >= 64 && tid < 128) {
#pragma unroll
        for (int k = 0; k < NC; ++k) lds[k * 128 + (tid - 64)] = acc[k];
    }
    __syncthreads();
    if (tid < 64) {                                                     // wave 0, all of its lanes
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            double v = combine(k, acc[k], lds[k * 128 + tid]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = combine(k, v, __shfl_down(v, off));
            acc[k] = v;
        }
    }
}

template <typename P>
__global__ __launch_bounds__(NG_REDUCE_THREADS) void ng_reduce_parts_kernel(const P p, int64_t n, double* parts) {
    __shared__ double lds[P::cols * 128];
    double acc[P::cols];
#pragma unroll
    for (int k = 0; k < P::cols; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * NG_REDUCE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NG_REDUCE_THREADS)
        p.add(i, acc);
    ng_fold<P::cols>(acc, lds, typename P::Combine());
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < P::cols; ++k) parts[(size_t)blockIdx.x * P::width + P::column(k)] = acc[k];
    }
}

template <typename P>
__global__ __launch_bounds__(NG_REDUCE_THREADS) void ng_reduce_finish_kernel(const double* parts, int n_parts, double* row) {
    __shared__ double lds[P::cols * 128];
    const int tid = threadIdx.x;
    const typename P::Combine combine;
    double acc[P::cols];
#pragma unroll
    for (int k = 0; k < P::cols; ++k) acc[k] = 0.0;
    for (int i = tid; i < n_parts; i += NG_REDUCE_THREADS) {
#pragma unroll
        for (int k = 0; k < P::cols; ++k) acc[k] = combine(k, acc[k], parts[(size_t)i * P::width + P::column(k)]);
    }
    ng_fold<P::cols>(acc, lds, combine);
    // the places of the row that are no column's: zeros, written by threads that own nothing else
    if (P::width > P::cols && tid >= 64 && tid < 64 + P::width) {
        bool mine = false;
#pragma unroll
        for (int k = 0; k < P::cols; ++k) mine = mine || P::column(k) == tid - 64;
        if (!mine) row[tid - 64] = 0.0;
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < P::cols; ++k) row[P::column(k)] = acc[k];
    }
}

// n elements by `blocks` workgroups (nd_reduce_blocks(n): none for n == 0, and then the row is the empty sums) through
// `parts`, blocks x P::width doubles of the caller's scratch
template <typename P>
static inline void ng_reduce_launch(const P& p, int64_t n, int64_t blocks, double* parts, double* row, hipStream_t s) {
    if (blocks)
        hipLaunchKernelGGL(ng_reduce_parts_kernel<P>, dim3((unsigned)blocks), dim3(NG_REDUCE_THREADS), 0, s, p, n, parts);
    hipLaunchKernelGGL(ng_reduce_finish_kernel<P>, dim3(1), dim3(NG_REDUCE_THREADS), 0, s, parts, (int)blocks, row);
}
