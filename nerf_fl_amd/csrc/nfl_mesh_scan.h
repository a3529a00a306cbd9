// nfl_mesh_scan.h -- what the mesh translation units share: launch sizes, size checks and the library's prefix sum.
// nm_scan and nm_scan_bytes are defined in nfl_mesh.hip, next to their kernels; nfl_simplify.hip calls them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define NM_THREADS 256
#define NM_SCAN_THREADS 512
#define NM_SCAN_ITEMS 4
#define NM_SCAN_TILE (NM_SCAN_THREADS * NM_SCAN_ITEMS)      // 2048: 2^31 elements -> 2^20 -> 2^9 -> 1 tile sums
#define NM_SCAN_LEVELS 3

typedef int64_t i64;

#define NM_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define NM_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

static inline size_t nm_pad(size_t bytes) { return (bytes + 15) / 16 * 16; }
static inline i64 nm_cdiv(i64 a, i64 b) { return (a + b - 1) / b; }
static inline unsigned nm_grid(i64 n) { return (unsigned)nm_cdiv(n, NM_THREADS); }
static inline bool nm_sizes_ok(i64 V, i64 T) { return V >= 0 && T >= 0 && V <= INT32_MAX && T <= INT32_MAX / 3; }
static inline bool nm_launched() { return hipGetLastError() == hipSuccess; }
static inline size_t nm_max(size_t a, size_t b) { return a > b ? a : b; }

__device__ __forceinline__ bool nm_in_range(int32_t a, int32_t b, int32_t c, i64 V) {
    return a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
}

// tile sums of all levels above the elements themselves, 8 B each
size_t nm_scan_bytes(i64 n);
// out (n) int64 = exclusive prefix sums of in (n) int32, *total = their sum; `sums`: nm_scan_bytes(n) of scratch
void nm_scan(const int32_t* in, i64* out, i64 n, i64* sums, i64* total, hipStream_t s);
