// nfl_geom.h -- what the geometry translation units share on the device side (every unit that makes, cleans, simplifies,
// smooths, colours, renders, fuses, measures, registers, closes or casts rays against a lattice or a mesh: nfl_surface, nfl_mesh,
// nfl_mesh_scan, nfl_occupancy, nfl_simplify, nfl_meshsmooth, nfl_tsdf, nfl_meshdist, nfl_register, nfl_meshcast, nfl_meshedge, and through
// nfl_meshray.h nfl_meshcolor, nfl_meshrender and nfl_atlas): launch sizes, the finite test, the splitmix64 hash, the fetch of
// an fp32 triangle and its face normal, the triangle grid's cell function and faces, the workgroup prefix sum, the library's
// tiled scan and the small pieces of the mesh kernels.  The scratch layouts, the size checks and the pointer checks are host
// arithmetic and live in nfl_geom_layout.h; the fixed-order fp64 reduction is nfl_reduce.h.  DESIGN.md sections 22 and 35.
#pragma once
#include <hip/hip_runtime.h>

#include "nfl_geom_layout.h"

#define NM_THREADS 256

#define NM_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define NM_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

static inline unsigned nm_grid(i64 n) { return (unsigned)ng_cdiv(n, NM_THREADS); }
static inline bool ng_launched() { return hipGetLastError() == hipSuccess; }

__device__ __forceinline__ bool nm_in_range(int32_t a, int32_t b, int32_t c, i64 V) {
    return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

// neither an infinity nor a NaN.  The same answer as isfinite on every input: nothing here is built with fast-math
__device__ __forceinline__ bool ng_is_finite(float x) { return x - x == 0.f; }
__device__ __forceinline__ bool ng_is_finite(double x) { return x - x == 0.0; }

// the finaliser of splitmix64, every input bit reaches every output bit: the hash of the simplify tables and of the surface
// sampler's draws
__device__ __forceinline__ uint64_t ng_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the corners of triangle t of an fp32 mesh; false when an index is out of range or a coordinate is not finite
__device__ __forceinline__ bool nm_corners(const float* ver, const int32_t* tri, i64 V, i64 t, float* a, float* b, float* c) {
    const int32_t ia = tri[3 * t], ib = tri[3 * t + 1], ic = tri[3 * t + 2];
    if (!nm_in_range(ia, ib, ic, V)) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = ver[3 * (i64)ia + k];
        b[k] = ver[3 * (i64)ib + k];
        c[k] = ver[3 * (i64)ic + k];
        ok = ok && ng_is_finite(a[k]) && ng_is_finite(b[k]) && ng_is_finite(c[k]);
    }
    return ok;
}

// cr = (b - a) x (c - a) and its length, every operation rounded on its own; cr / len is the unit face normal.  What len
// must be for the triangle to count is the caller's: the sampler, nfl_mesh_closest's d_dot and the registration differ.
__device__ __forceinline__ void nm_face_cross(const float* a, const float* b, const float* c, float* cr, float* len) {
    const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    cr[0] = ab[1] * ac[2] - ab[2] * ac[1];
    cr[1] = ab[2] * ac[0] - ab[0] * ac[2];
    cr[2] = ab[0] * ac[1] - ab[1] * ac[0];
    *len = sqrtf((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
}

// THE GRID of "mesh distance": what nfl_meshdist (which builds it and finds closest points in it) and nfl_meshcast (which
// walks rays through it) share, so that both mean the same cells
struct NdGrid {
    float lo[3];
    float cell;
    int32_t dims[3];
};

static inline bool nd_grid_ok(const float* lo, float cell, const int32_t* dims) {
    if (!nd_dims_ok(dims) || !(cell > 0.f) || !ng_finite(cell)) return false;
    return ng_finite(lo[0]) && ng_finite(lo[1]) && ng_finite(lo[2]);
}

static inline NdGrid nd_grid_of(const float* lo, float cell, const int32_t* dims) {
    return {{lo[0], lo[1], lo[2]}, cell, {dims[0], dims[1], dims[2]}};
}

__device__ __forceinline__ int nd_cellf(float x, float lo, float cell, int n) {
    return (int)fminf(fmaxf(floorf((x - lo) / cell), 0.f), (float)(n - 1));
}

// the face at index i of an axis that starts at lo, in fp64: F = lo + i * cell, and its explicit slack S = 2^-21 * (|lo| + i * cell).
// cellf is computed in fp32, and the smallest x with cellf(x) >= i lies within S of F
__device__ __forceinline__ void nd_face(float lo32, float cell, int i, double* F, double* S) {
    const double lo = (double)lo32, ic = (double)i * (double)cell;
    *F = lo + ic;
    *S = 4.76837158203125e-07 * (fabs(lo) + ic);                                        // 2^-21
}

// adds the wave's number of `bad` lanes to *counter: one atomic per wave that has any.  Every lane must call it.
__device__ __forceinline__ void ng_count_bad(bool bad, i64* counter) {
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == __ffsll(m) - 1) atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)__popcll(m));
}

// vertex rows of a mesh (positions, normals, colours) and where their survivors go; a null input row is absent
struct NgRows {
    const float* in[3];
    float* out[3];
};

template <typename T>
__device__ __forceinline__ T ng_shfl_up(T v, int off) { return __shfl_up(v, off); }

// Exclusive prefix sum of v over the THREADS threads of the workgroup (wave shuffle-up, the wave sums through LDS, the
// sums of the waves before added); total = the sum over the workgroup.  T: an integer, or a struct with +, - and an
// ng_shfl_up of its own.  `wave_sum` is THREADS / 64 entries of LDS; every thread calls.  A kernel that calls again with
// the same wave_sum puts a barrier between the calls (the waves of this call are still reading it).
template <typename T, int THREADS>
__device__ __forceinline__ T ng_block_scan(T v, T* wave_sum, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = ng_shfl_up(incl, off);
        if (lane >= off) incl = incl + up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    T before = T(), all = T();
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const T s = wave_sum[w];
        if (w < wave) before = before + s;
        all = all + s;
    }
    total = all;
    return before + incl - v;
}

// nfl_mesh_scan.hip.  out (n) int64 = exclusive prefix sums of in (n) int32, *total = their sum, by tiles of NM_SCAN_TILE
// elements over up to NM_SCAN_LEVELS levels; `sums`: nm_scan_bytes(n) of scratch
void nm_scan(const int32_t* in, i64* out, i64 n, i64* sums, i64* total, hipStream_t s);
// ids[v] = rank[ids[v]] where ids[v] >= 0: from the smallest member of a group (a root, a leader) to the group's number
void nm_rank(int32_t* ids, i64 n, const i64* rank, hipStream_t s);

// Writes the flagged triangles, re-indexed through `map` (int64 offsets of kept vertices, or int32 cluster ids).  What is
// read from the scratch, `map` and `tri` is checked like any other index, so a scratch that is not the count call's makes
// a triangle be skipped, never read or written out of range.
template <typename Tmap>
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_emit_triangles_kernel(const int32_t* flag, const i64* off, const int32_t* tri,
                                                                             const Tmap* map, i64 V, i64 T, i64 n_out_v, i64 n_out_t,
                                                                             int32_t* out) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (t >= T || !flag[t]) return;                         // a flagged triangle has its three indices in range and kept
    const i64 o = off[t];
    if (o < 0 || o >= n_out_t) return;
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (!nm_in_range(a, b, c, V)) return;
    const Tmap na = map[a], nb = map[b], nc = map[c];
    if (na < 0 || nb < 0 || nc < 0 || na >= n_out_v || nb >= n_out_v || nc >= n_out_v) return;
    out[3 * o] = (int32_t)na;
    out[3 * o + 1] = (int32_t)nb;
    out[3 * o + 2] = (int32_t)nc;
}
